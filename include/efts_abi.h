/*
 * efts_abi.h -- C ABI of libefts_hip.so: the MI355X (gfx950) implementation of the
 * EFTS-CNN acoustic-model hot path.
 *
 * The reference (liusongxiang/efficient_tts) is pure Python/PyTorch and has NO FFI or
 * plugin interface; its boundary for this path is the Python class
 * nntts.models.EfficientTTSCNN (nntts/models/efficient_tts.py:23) resolved by name at
 * nntts/bin/train.py:173-185.  This header therefore defines the C entry points a
 * maintainer would bind (ctypes) to replace the stock torch ops that class calls; each
 * entry cites the reference op(s) it replaces.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers + explicit sizes; no torch types, no hidden allocation,
 *     no retained pointers.  The caller owns every buffer.
 *   - every launch goes to the hipStream_t passed as `void* stream`; no device sync.
 *   - return 0 on success, negative EFTS_E* on error; efts_last_error() gives the text
 *     (thread-local).  Nothing throws across the ABI.
 *
 * Row space.  Activations of B items x T steps live in a padded, item-major row space:
 *   row(b, t) = b * Tp + t,  Tp = T + EFTS_GAP, rows t >= T of every item are zero ("gap").
 * With a gap of (k-1)/2 = 2 zero rows between items a 1-D convolution over the whole
 * row space equals B independent zero-padded convolutions, so tiles may straddle items.
 * Buffers carry EFTS_GUARD_LO zero rows before row 0 and EFTS_GUARD_HI rows after the
 * last 128-row tile; pointers passed in point at row 0.
 *
 * MFMA operand planes.  Matrices consumed by the MFMA GEMM are row-major, K in 128-byte
 * chunks; the format is named by a `split` value (EFTS_SPLIT_*):
 *   split 1 ("bf16")   : row = [Kp] bf16,            Kp = roundup(K, 64); chunk = 64 k's
 *   split 2 ("bf16x3") : row = [Kp/32][hi32 | lo32], Kp = roundup(K, 32); chunk = 32 k's,
 *                        x = hi + lo (two bf16), product = hi*hi + hi*lo + lo*hi in fp32.
 *   split 3 ("fp32")   : row = [Kp] fp32,            Kp = roundup(K, 32); chunk = 32 k's,
 *                        the exact value; efts_gemm contracts it on v_mfma_f32_32x32x2_f32
 *                        (a k-ordered fmaf chain, no operand rounding).  Same chunk geometry as
 *                        split 2, so nchunk, row strides and guard rows are unchanged.  Produced
 *                        and consumed by the eval-path entry points; the fused kernels
 *                        (efts_resconv5, efts_frame_linear, efts_expand, efts_embed_conv) and
 *                        the training entry points have no fp32 form and refuse it (EFTS_EINVAL).
 */
#ifndef EFTS_ABI_H
#define EFTS_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EFTS_GAP 2
#define EFTS_GUARD_LO 8
#define EFTS_GUARD_HI 144
#define EFTS_TILE_M 128

#define EFTS_OK 0
#define EFTS_EINVAL (-1)
#define EFTS_ESHAPE (-2)
#define EFTS_EALIGN (-3)
#define EFTS_ELAUNCH (-4)
#define EFTS_EDEVICE (-5)

#define EFTS_SPLIT_BF16 1
#define EFTS_SPLIT_BF16X3 2
#define EFTS_SPLIT_FP32 3

#define EFTS_ACT_NONE 0
#define EFTS_ACT_LEAKY 1 /* LeakyReLU, slope in args */
#define EFTS_ACT_RELU 2
#define EFTS_ACT_TANH 3 /* the vocoder's output layer */

/* ABI revision of THIS header.  Bumped whenever an argument block changes size / meaning or an export is removed, so that a consumer built
 * against another revision can tell: efts_version() returns the revision the library was built from, and a binding must refuse to run unless
 * it equals the EFTS_ABI_VERSION it was written against (efficient_tts_amd/lib.py does, tests/test_abi_cpu.py pins all three).
 *   100  rounds 1-4
 *   500  round 5: efts_resconv5_args grew by act_bwd_sign / act_bwd_bias_part / act_bwd_bias_rows / act_bwd_slope / kernel;
 *        efts_wgrad_tn, efts_wgrad_reduce_bias, efts_resconv5_kernel removed (efts_wgrad_tn_grouped / efts_wgrad_reduce_grouped instead)
 *   600  round 6: + efts_frame_pack_dit, efts_logmel_dit; efts_pack_item.plane may be NULL (dgrad plane only)
 *   601  round 6: efts_gemm_args grew by sqerr_target / ld_target / target_batch_stride / sqerr_part;
 *        + efts_losses_from_parts, efts_logmel_fft, efts_logmel_fft_pcm16
 *   602  (this header): operand format 3 (EFTS_SPLIT_FP32); efts_reconst_alpha and efts_pack_vt take the format of their plane
 *        + efts_gl_init, efts_gl_synthesis, efts_gl_analysis, efts_gl_overlap_add (Griffin-Lim vocoder): exports added, nothing that existed
 *        changed size or meaning, so by the rule above the revision stays (a binding that needs them and meets an older library fails on the
 *        missing symbol)
 *        + efts_optim_step, efts_optim_hyper (Adam / AdamW / RAdam): exports added, the revision stays by the same rule
 *        + efts_resample, efts_resample_pcm16 (sample-rate conversion): exports added, the revision stays by the same rule
 *        + efts_mel_cepstrum, efts_dtw (scoring synthesis against a recording): exports added, the revision stays by the same rule
 *        + efts_yin, efts_yin_pcm16 (pitch tracking), efts_dtw_path, efts_dtw_path_workspace_bytes, efts_f0_path_error (the warping path and
 *          the F0 error along it): exports added, the revision stays by the same rule
 *        + efts_trim, efts_trim_pcm16, efts_trim_workspace_bytes (silence trimming and peak normalisation): exports added, the revision stays
 *          by the same rule
 *        + efts_f0_viterbi, efts_f0_viterbi_workspace_bytes (pitch smoothing across frames): exports added, the revision stays by the same
 *          rule
 *        + efts_stft_mag, efts_stft_dist, efts_stft_dist_workspace_bytes (STFT magnitudes at four sizes and the multi-resolution STFT
 *          distance): exports added, the revision stays by the same rule
 *        + efts_loudness, efts_loudness_pcm16, efts_loudness_workspace_bytes (BS.1770 integrated loudness and the gain to a target):
 *          exports added, the revision stays by the same rule
 *        + efts_denoise, efts_denoise_workspace_bytes (spectral subtraction of a vocoder's bias noise): exports added, the revision stays
 *          by the same rule
 *        + efts_stoi, efts_stoi_workspace_bytes (STOI and ESTOI intelligibility scores): exports added, the revision stays by the same
 *          rule
 *        + efts_logspec_project, efts_frame_dist (waveform mel-cepstra and the distance between frames paired one to one): exports added,
 *          the revision stays by the same rule
 *        + efts_noise_profile, efts_noise_profile_workspace_bytes, efts_spectral_gate (a noise profile per recording and the spectral gate
 *          that uses it): exports added, the revision stays by the same rule
 *        + efts_true_peak, efts_true_peak_pcm16, efts_peak_limit, efts_peak_limit_pcm16, efts_limiter_workspace_bytes (true-peak metering
 *          and the look-ahead peak limiter): exports added, the revision stays by the same rule
 *        + efts_ema_update, efts_ema_hyper (exponential moving average of the parameters): exports added, the revision stays by the same
 *          rule
 *        + efts_iir, efts_iir_pcm16, efts_iir_workspace_bytes (a cascade of second-order sections with exact state carry): exports added,
 *          the revision stays by the same rule
 *        + efts_pauses, efts_pauses_pcm16, efts_pauses_workspace_bytes (shortening the long pauses inside a recording): exports added, the
 *          revision stays by the same rule
 *        + efts_resblock2 (one HiFi-GAN ResBlock2, two dilated convolutions fused through LDS): export added, the revision stays by the
 *          same rule
 *        + efts_istft_head (the inverse-STFT head of an iSTFTNet generator): export added, the revision stays by the same rule
 *        + efts_snake_aa (BigVGAN's anti-aliased Snake / SnakeBeta activation): export added, the revision stays by the same rule */
#define EFTS_ABI_VERSION 602
int efts_version(void);
const char* efts_last_error(void);
/* 0 when the current HIP device is gfx950. */
int efts_device_check(void);

/* ------------------------------------------------------------------------------------
 * The MFMA contraction: out = epilogue( alpha * sum_tap A[row + tap - pad, :] . Bw[tap][col, :] )
 * Replaces torch Conv1d (nntts/layers/efts_modules.py:32-35,48-51; duration_predictor.py:57),
 * Linear (efficient_tts.py:149-153,161,198) and bmm (efficient_tts.py:190,390).
 * epilogue: + bias[col]; activation; + resid[row, col]; * rowmask[row]; store fp32 and/or
 * bf16 operand plane(s) for the next contraction.
 * ---------------------------------------------------------------------------------- */
typedef struct efts_gemm_args {
    /* A operand plane (activations): row 0 pointer, row stride in bytes */
    const void* a;
    int64_t lda;
    int64_t a_batch_stride; /* bytes between batch items (batched mode), else 0 */
    /* B operand plane ("weights"): [taps][N rows][K], row stride / tap stride in bytes */
    const void* b;
    int64_t ldb;
    int64_t b_tap_stride;
    int64_t b_batch_stride;
    int32_t split;  /* 1 = bf16, 2 = bf16x3 (hi/lo interleaved), 3 = fp32 (generic tiling only) */
    int32_t taps;   /* 1, 3, 5, 7, 9 or 11 */
    int32_t m;      /* rows per batch item */
    int32_t n;      /* output columns */
    int32_t nchunk; /* 128-byte K chunks per row */
    int32_t batch;  /* >= 1 */
    float alpha;
    int32_t act;
    float slope;
    const float* bias;    /* [n] or NULL */
    const float* resid;   /* fp32 [m, ldr] or NULL */
    int64_t ldr;          /* elements */
    int64_t resid_batch_stride;
    const float* rowmask; /* fp32 [m] (per batch item: + z*m_mask_stride) or NULL */
    int64_t rowmask_batch_stride;
    float* out_f32; /* or NULL */
    int64_t ldo;    /* elements */
    int64_t out_batch_stride;
    void* out_bf16;    /* operand plane for the next contraction, or NULL */
    int64_t ldob;      /* bytes */
    int64_t outb_batch_stride;
    int32_t out_split; /* 1, 2 or 3: format of out_bf16 */
    int32_t batch2;    /* optional outer batch (grid.z), 0/1 = none; e.g. the taps of a wgrad */
    int64_t a_batch2_stride, b_batch2_stride, out_batch2_stride; /* bytes, bytes, elements */
    /* dilated convolutions (HiFi-GAN residual blocks, nntts/vocoders/hifigan_model.py:30-58): rows between taps,
     * 0 / 1 = dense; (taps - 1) * dilation <= 64; taps may also be 7 or 11.  The A plane is read from
     * (taps - 1) / 2 * dilation rows before row 0 to 144 rows after row m - 1: the caller's buffer must hold zero rows
     * there (EFTS_GUARD_LO = 8 covers the dense taps of the acoustic model; the vocoder's row spaces carry 64). */
    int32_t dilation;
    /* 1: out_bf16 receives LeakyReLU(out, plane_slope) instead of out -- for consumers that apply the
     * activation to their INPUT (pre-activation residual blocks); out_f32 stays un-activated. */
    int32_t plane_act;
    float plane_slope;
    /* out_split 1 only, optional: a second plane of the layout of out_bf16 that receives the bf16 REMAINDER
     * out - bf16(out), so that a consumer can rebuild out to 16 mantissa bits (the residual input of efts_resconv5). */
    void* out_bf16_lo;
    /* which of the (bit-identical) kernels runs: EFTS_TILING_AUTO picks by shape; the explicit values are for A/B timing and
     * for the equality tests between the kernels (EFTS_TILING_SMALLM excepted, see below).  An explicit tiling the shape does not allow is an error. */
    int32_t tiling;
    /* training forward of a LeakyReLU / ReLU layer: the sign of every activated output BEFORE the residual add, as bit words
     * for efts_act_bwd mode 4 (instead of keeping y and x in fp32 for the backward: 1/8 B instead of 8 B per element read
     * there).  Row stride n / 8 bytes; within a row, 16 bytes per 128-column group: word u (0..3), bit q (0..31) = column
     * 128 * group + 4 * q + u is positive.  Needs n % 128 == 0, batch 1, 16-byte aligned fp32 / plane rows (the vector epilogue),
     * and runs on the generic or wide tiling only.  NULL: not written. */
    void* sign_mask;
    /* attention scores -> expected key index in the epilogue (scaled_dot_product_attention + the soft index of imv_generator,
     * nntts/models/efficient_tts.py:391-398, :312): soft_index[b][row] = sum_i i * softmax_i(out[b][row][i < key_len[b]]) for
     * row < query_len[b], 0 beyond -- what efts_attn_soft_index computes from the stored scores, without storing them
     * (out_f32 may be NULL then).  Needs n <= 128 (one column tile holds a whole row), generic tiling, no residual / plane
     * outputs.  soft_index: fp32 [batch][m]; key_len, query_len: int32 [batch].  NULL: not computed. */
    float* soft_index;
    const int32_t* key_len;
    const int32_t* query_len;
    /* train-mode Dropout on the activated value, BEFORE the residual add (ResConv1d / mel_prenet with dropout_rate > 0,
     * nntts/layers/efts_modules.py:38-47, efficient_tts.py:76-80): element (row, col) is kept and scaled by 1 / (1 - drop_p) iff
     * hash(drop_seed, row * n + col) >= drop_p * 2^32 -- a stateless counter-based mask efts_act_bwd_dropout regenerates (not
     * torch's Philox stream: same distribution, different draws).  batch 1, generic / wide tiling, vector epilogue.  0: none. */
    float drop_p;
    uint32_t drop_seed;
    /* the mel term of FastSpeechLoss in the epilogue of the mel head (nntts/losses/fastspeech_loss.py:54-67 behind
     * nntts/models/efficient_tts.py:198-200, :220): per workgroup and wave, the sum of (out - target)^2 over the rows of the tile whose
     * rowmask value is not zero -- sqerr_part[((batch item * row tiles) + row tile) * 4 + wave], row tiles = ceil(m / 128) --
     * in a fixed order (deterministic; efts_losses_from_parts adds the partial sums up).  target: fp32 [batch][m][ld_target] (what the
     * caller padded the frames with is never read past a zero rowmask value); needs rowmask, one tap, n <= 128, n % 4 == 0, no residual,
     * no dropout, 16-byte aligned target rows, and runs on the generic tiling only.  NULL: not computed. */
    const float* sqerr_target;
    int64_t ld_target;           /* elements */
    int64_t target_batch_stride; /* elements */
    float* sqerr_part;
} efts_gemm_args;

#define EFTS_TILING_AUTO 0
#define EFTS_TILING_GENERIC 1  /* 124-row x 128-column tiles, two 4-wave workgroups per CU: every shape */
#define EFTS_TILING_WIDE 2     /* 252-row x 128-column tiles: dense k5 launches */
#define EFTS_TILING_NARROW 3   /* 64- / 32-column tiles */
#define EFTS_TILING_RESIDENT 4 /* window + all taps resident in LDS: n <= 64, one K chunk, taps 3 / 7 / 11 */
#define EFTS_TILING_SMALLM 5   /* short row spaces (one utterance): 64 x 32 tiles, K split across the four waves, operand fragments
                                * straight from global memory; taps 1 / 3 / 5, batch 1, n % 32 == 0, the A plane readable up to the next
                                * multiple of 64 rows (+ pad).  Same operand rounding as the other tilings but a different summation
                                * order (equal to fp32 rounding, not bit for bit): never chosen by AUTO, the caller asks for it */

int efts_gemm(const efts_gemm_args* a, void* stream);

/* ------------------------------------------------------------------------------------
 * One residual convolution layer of the EFTS-CNN stacks (ResConv1d.forward,
 * nntts/layers/efts_modules.py:48-51 with the Conv1d k=5 of :32-35; the stack loop is :77-79):
 *   y[row, :] = ( x[row, :] + LeakyReLU( conv1d_k5(x)[row, :] + bias, slope ) ) * rowmask[row]
 * on a padded row space, for long row spaces (the mel-length stacks).  The contraction runs on the operand plane `x`
 * (format `split`); the RESIDUAL x is taken, in this order, from x_f32 (fp32 [m][ldr]) if given, else from the
 * planes as hi + lo: split 2 planes carry lo inside x; a split 1 plane may come with a separate lo plane x_lo of the
 * same layout (NULL: the residual is the bf16 value itself).  A residual from the planes needs planes of at least
 * n columns: nchunk * 64 (split 1) or nchunk * 32 (split 2) < n without x_f32 and without no_residual is EFTS_ESHAPE.
 * Outputs, any combination: y (operand plane of format y_split; with y_split 1 an optional lo plane y_lo so that the
 * next layer can rebuild its residual), y_f32.
 * Bit-identical to efts_gemm(taps 5, LeakyReLU, resid, rowmask) on the same operands.
 * n (= cout) must be a multiple of 256; x is read from 2 rows before row 0 to 144 rows after row m - 1 (the guard rows).
 * ---------------------------------------------------------------------------------- */
typedef struct efts_resconv5_args {
    const void* x;      /* operand plane of the layer input, row 0 */
    const void* x_lo;   /* split 1 only: bf16 remainder plane of x, or NULL */
    int64_t ldx;        /* bytes, both planes */
    const float* x_f32; /* fp32 residual stream or NULL */
    int64_t ldr;        /* elements */
    const void* w;      /* B operand plane [5][n][K] (efts_pack_weight) */
    int64_t ldw;
    int64_t w_tap_stride;
    int32_t split;      /* format of x and w: 1 = bf16, 2 = bf16x3 */
    int32_t m;          /* rows */
    int32_t n;          /* output channels, % 256 == 0 */
    int32_t nchunk;     /* 128-byte K chunks per row of x / w */
    const float* bias;  /* [n] or NULL */
    float slope;        /* LeakyReLU slope */
    const float* rowmask; /* [m] or NULL */
    float* y_f32;       /* fp32 [m][ldo] or NULL */
    int64_t ldo;        /* elements */
    void* y;            /* operand plane of the layer output or NULL */
    void* y_lo;         /* y_split 1 only: remainder plane of y, or NULL */
    int64_t ldy;        /* bytes, both planes */
    int32_t y_split;    /* 1 or 2 */
    const int32_t* plan; /* HOST pointer: explicit tile schedule (format of efts_resconv5_plan) or NULL = automatic */
    int32_t taps;        /* 0 / 5: the k5 layer; 3: a k3 convolution with a [3][n][K] weight plane (duration_predictor.py:57, or a
                          * ResConv1d stack built with k_size = 3) on the same kernel: window and tile geometry of the k5 layer */
    int32_t no_residual; /* 1: y = LeakyReLU(conv + bias, slope) * rowmask without the residual term (slope 0 = ReLU): the
                          * duration predictor's Conv1d + ReLU, riding in a decoder launch (efts_resconv5_multi) */
    void* sign_bits;     /* training forward, optional: the sign of every activated output BEFORE the residual add as plain bit rows for
                          * efts_act_bwd mode 5 -- row stride n / 8 bytes, bit j of byte c = column 8 c + j is positive (the same
                          * information as efts_gemm_args.sign_mask, in the order this kernel's epilogue holds it).  NULL: not written */
    /* training backward, optional: this launch is the DGRAD of stack layer l -- x = the operand plane of dZ_l, w = the transposed weights,
     * x_f32 = G, y_f32 = G' = d loss / d x_l, slope 1, no bias -- and its epilogue also runs the activation backward of layer l - 1
     * (efts_act_bwd mode 5 | EFTS_ACT_BWD_BIAS_PARTS) on the values it holds: y receives dZ_{l-1} = G' * (bit ? 1 : act_bwd_slope) as an
     * operand plane of format y_split = split, act_bwd_bias_part one row of column sums of dZ_{l-1} per tile and wave row
     * (efts_resconv5_bias_rows(m, n) rows of n floats; every row is written by every launch -- rows of tiles the schedule does not have
     * receive zeros -- so the table needs no clearing and may be re-used across shapes; NULL: no sums).  act_bwd_sign = the sign_bits layer l - 1's forward launch wrote.  NULL: a plain layer. */
    const void* act_bwd_sign;
    float* act_bwd_bias_part;
    int32_t act_bwd_bias_rows;
    float act_bwd_slope;
    int32_t kernel;      /* which kernel runs the launch (every layer of a grouped launch must name the same one; other values: EFTS_EINVAL).
                          * 0: the 8-wave ping-pong kernel -- the
                          * product path.  2: the one-wave-per-SIMD kernel with the generated main loop wherever it applies (bf16 planes, 5 taps,
                          * >= 2 K chunks, no fused activation backward; the 8-wave kernel elsewhere): same results bit for bit, same time on
                          * MI355X (DESIGN.md 4a'), kept for the bit-equality tests between the two and for A/B measurements */
} efts_resconv5_args;

int efts_resconv5(const efts_resconv5_args* a, void* stream);
/* rows of efts_resconv5_args.act_bwd_bias_part for an m x n layer on the current device (the automatic schedule) */
int efts_resconv5_bias_rows(int32_t m, int32_t n);

/* `count` (1 or 2) independent residual layers of the same geometry (split, n, nchunk, ldw) in ONE persistent launch: the rows of
 * the layers are laid end to end and scheduled over the compute units as one row space; a tile never crosses from one layer
 * into the next, and every tile brings its own operands, weights, bias, mask and outputs.  This is how a short stack rides
 * along with a long one -- text-encoder layer k + 2 (64 x 130 rows) in the launch of mel-encoder layer k (64 x 802 rows;
 * nntts/models/efficient_tts.py:148 and :162 are independent until :167) -- at the long launch's efficiency instead of a
 * launch of its own that cannot fill the chip.  Results per layer are those of efts_resconv5.  layers[0].plan (optional)
 * schedules the combined rows. */
int efts_resconv5_multi(const efts_resconv5_args* layers, int32_t count, void* stream);

/* A Linear with few input features applied to the caller's fp32 frames, written into the row space:
 *   y[b * Tp + t, :] = act(x[b][t][:cin] . W^T + bias), t < T (rows t >= T of the row space are not touched: they stay zero)
 * -- `mel_prenet` of the reference (nntts/models/efficient_tts.py:76-80, applied at :161; eval / Dropout-free) in one launch,
 * without an operand plane of the input.  Bit-identical to efts_pack_rows + efts_gemm.  cin % 8 == 0, cin <= 128, n % 128 == 0. */
typedef struct efts_frame_linear_args {
    const float* x;      /* [B][T][cin] fp32, contiguous, 16-byte aligned */
    const void* w;       /* packed B plane [n][ldw] (efts_pack_weight, one tap) of format `split` */
    int64_t ldw;
    int32_t split;       /* operand format the contraction runs in: 1 bf16, 2 bf16x3 (hi / lo) */
    const float* bias;   /* [n] or NULL */
    int32_t act;         /* EFTS_ACT_* */
    float slope;
    int32_t B, T, Tp, cin, n;
    float* y_f32;        /* [B * Tp][ldo] or NULL */
    int64_t ldo;         /* floats */
    void* y;             /* operand plane of the output (row 0) or NULL */
    void* y_lo;          /* y_split 1 only: bf16 remainder plane or NULL */
    int64_t ldy;         /* bytes, both planes */
    int32_t y_split;
    int32_t max_workgroups; /* 0: one workgroup per (item, 128-channel slice); > 0: at most this many (each then takes several units in
                             * turn), leaving compute units to a launch that runs beside this one -- the kernel is HBM-bound */
} efts_frame_linear_args;
int efts_frame_linear(const efts_frame_linear_args* a, void* stream);

/* The static tile schedule of efts_resconv5 for m rows x n columns on `cus` compute units (0: the current device).
 * One persistent workgroup per CU; the workgroups form groups (one workgroup per 256-column tile); group g belongs to
 * class g % classes and owns `rows` consecutive output rows, cut into `ntile` tiles of 32 * h - 4 rows, h = 2..8 half
 * units of 32 window rows (odd heights: the two wave rows of the workgroup take ceil(h/2) and floor(h/2) 32-row blocks).
 * plan (host memory, >= EFTS_RC_PLAN_INTS int32) = [groups, classes, then for each of 4 classes: rows, ntile, h[8]].
 * Returns the number of int32 written, or a negative EFTS_E* code.  No device work. */
#define EFTS_RC_PLAN_INTS 42
int efts_resconv5_plan(int32_t m, int32_t n, int32_t cus, int32_t* plan, int32_t cap);

/* ------------------------------------------------------------------------------------
 * Parameter preparation.
 * efts_pack_weight: w[cout][cin][taps] fp32 (torch Conv1d / Linear layout) -> B operand plane
 * [taps][cout][Kp].  With g != NULL the weight-norm fold w = g * v / ||v|| (norm over cin*taps)
 * is applied first (torch.nn.utils.weight_norm, nntts/layers/efts_modules.py:92-99;
 * remove_weight_norm efficient_tts.py:400-409); w_f32_out (optional) receives the folded fp32
 * weight in the input layout.  plane row stride = ldb bytes, tap stride = cout*ldb.
 * ---------------------------------------------------------------------------------- */
int efts_pack_weight(const float* w, const float* g, float* w_f32_out, void* plane, int64_t ldb,
                     int32_t cout, int32_t cin, int32_t taps, int32_t split, void* stream);

/* ------------------------------------------------------------------------------------
 * Row-space producers.  `rows` = B*Tp.  f32_out (optional) is [rows][c] fp32, plane (optional)
 * an A operand plane with row stride ld_plane bytes.  Gap rows are written as zero.
 * efts_row_masks : gapmask[row] = t < T ; lenmask[row] = t < len[b]
 *                  (make_non_pad_mask, nntts/utils/nets_utils.py:170-254, built on device).
 * efts_embed     : text_embedding_table(text) (efficient_tts.py:144); ids int64 [B,T].
 * efts_pack_rows : x fp32 [B,T,c] contiguous (e.g. speech [B,T2,80], efficient_tts.py:161 input).
 * ---------------------------------------------------------------------------------- */
int efts_row_masks(const int32_t* lengths, float* gapmask, float* lenmask, int32_t B, int32_t T,
                   int32_t Tp, void* stream);
/* both row spaces of a teacher-forced pass (text: T1, mel: T2) in ONE launch, straight from the caller's length tensors (int64 as
 * torch makes them -- is_int64 -- or int32): int32 copies of the lengths (what every later entry point takes) + the four masks. */
int efts_row_masks_pair(const void* len1, const void* len2, int32_t is_int64, int32_t* len1_i32, int32_t* len2_i32, float* gap1,
                        float* lenmask1, float* gap2, float* lenmask2, int32_t B, int32_t T1, int32_t Tp1, int32_t T2,
                        int32_t Tp2, void* stream);
int efts_embed(const int64_t* ids, const float* table, float* f32_out, void* plane, int64_t ld_plane,
               int32_t B, int32_t T, int32_t Tp, int32_t c, int32_t num_symbols, int32_t split,
               void* stream);
int efts_pack_rows(const float* x, float* f32_out, void* plane, int64_t ld_plane, int32_t B, int32_t T,
                   int32_t Tp, int32_t c, int32_t kp, int32_t split, void* stream);
/* Embedding AND the first residual convolution of the text encoder (efficient_tts.py:144 + the first ResConv1d of :148,
 * nntts/layers/efts_modules.py:48-51) as table look-ups: that layer's input takes only num_symbols distinct values per position and
 * the convolution is linear, so tap k's product with every symbol's embedding is tabulated once per weight set --
 * tap_table[k][v][:] = W_k . table[v] (fp32 [taps][num_symbols][c]; build it with `taps` one-tap efts_gemm launches over the
 * embedding rows, in the operand format the model runs in) -- and the layer becomes
 *   y[b * Tp + t] = table[id_t] + LeakyReLU( bias + sum_k tap_table[k][ id_{t + k - (taps-1)/2} ], slope )
 * with positions outside [0, lim) contributing nothing: lim = T (lengths NULL: padded ids are real symbols, the reference's
 * teacher-forced semantics) or lengths[b] (zero embedding and zero output beyond an item's length: batched free-running inference).
 * Same outputs as efts_embed (fp32 rows and / or operand plane, gap rows zero). */
int efts_embed_conv(const int64_t* ids, const int32_t* lengths, const float* table, const float* tap_table, const float* bias, float slope,
                    float* f32_out, void* plane, int64_t ld_plane, int32_t B, int32_t T, int32_t Tp, int32_t c, int32_t num_symbols,
                    int32_t taps, int32_t split, void* stream);

/* ------------------------------------------------------------------------------------
 * Alignment block (fp32 VALU, HBM-bound).
 * efts_attn_soft_index: scores[B][T2][ld] (= q.k/sqrt(D), from efts_gemm) -> softmax over the
 *   text_len[b] valid keys and soft_idx[b][j] = sum_i alpha_ij * i, 0 for j >= mel_len[b]
 *   (scaled_dot_product_attention :377-398 + mask :168 + the bmm of imv_generator :312).
 *   alpha_out (optional) [B][T1][T2] fp32 receives alpha itself.
 * efts_imv_scan: d_j = relu(s_j - s_{j-1}), d_0 = 0; pi = cumsum(d) * melmask;
 *   pi = pi / max(max_j pi, 1e-8) * (text_len - 1)            (imv_generator :314-323).
 * efts_aligned_positions: e[b][i] = sum_j softmax_j(-sigma_e (pi_j - p_i)^2) * q_j, masked
 *   (get_aligned_positions :326-345), and the duration target log(e_i - e_{i-1} + offset),
 *   0 at padded text (efficient_tts.py:203-216, delta_e_method_1).
 * efts_reconst_alpha: alpha'[b][i][j] = softmax_i(-sigma (q_j - e_i)^2), zero outside the
 *   text x mel mask (reconstruct_align_from_aligned_position :347-375 + :186).  Lengths NULL
 *   = inference (no masks, :270-274).  Writes the fp32 API tensor [B][T1][T2] (optional) and
 *   the A operand plane of alpha'^T, format `split` (2 or 3): row (b*T2p + j), K = i  (for the expand bmm :190).
 * efts_pack_vt: V fp32 [B*T1p][c] -> per-item B operand plane V^T [B][c][K = i], format `split` (2 or 3).
 * efts_cumsum_rows: e = cumsum(delta) over T1 (inference :260); x [B][T] contiguous.
 * ---------------------------------------------------------------------------------- */
int efts_attn_soft_index(const float* scores, int64_t ld, const int32_t* text_len, const int32_t* mel_len,
                         float* soft_idx, float* alpha_out, int32_t B, int32_t T1, int32_t T2, void* stream);
int efts_imv_scan(const float* soft_idx, const int32_t* text_len, const int32_t* mel_len, float* imv,
                  int32_t B, int32_t T2, void* stream);
int efts_aligned_positions(const float* imv, const int32_t* text_len, const int32_t* mel_len, float sigma_e,
                           float offset, float* e, float* log_delta_e, int32_t B, int32_t T1, int32_t T2,
                           void* stream);
/* the duration target alone: log(delta_e + offset) with delta_e_i = e_i - e_{i-1} (method1 != 0, efficient_tts.py:204) or
 * e_{i+1} - e_i with e_{len} = mel_len (method1 == 0, :205-213); 0 at padded text.  e, log_delta_e: [B][T1]. */
int efts_duration_target(const float* e, const int32_t* text_len, const int32_t* mel_len, float offset, int32_t method1,
                         float* log_delta_e, int32_t B, int32_t T1, void* stream);
int efts_reconst_alpha(const float* e, const int32_t* text_len, const int32_t* mel_len, float sigma,
                       float* alpha_out, void* plane, int64_t ld_plane, int32_t B, int32_t T1, int32_t T2,
                       int32_t T2p, int32_t split, void* stream);
int efts_pack_vt(const float* v, int64_t ldv, void* plane, int64_t ld_plane, int32_t B, int32_t T1,
                 int32_t T1p, int32_t c, int32_t split, void* stream);
int efts_cumsum_rows(const float* x, float* y, int32_t B, int32_t T, void* stream);

/* The middle of the alignment block in ONE launch (one workgroup per item, operands in LDS after the first load):
 * efts_imv_scan + efts_aligned_positions + efts_duration_target, bit-identical to that chain
 * (imv_generator efficient_tts.py:314-323, get_aligned_positions :326-345, duration target :203-216).
 * imv [B][T2], e [B][T1], log_delta_e [B][T1] or NULL.  2 * T2 floats must fit 160 KiB of LDS. */
int efts_imv_align(const float* soft_idx, const int32_t* text_len, const int32_t* mel_len, float sigma_e, float offset,
                   int32_t method1, float* imv, float* e, float* log_delta_e, int32_t B, int32_t T1, int32_t T2, void* stream);

/* Gaussian re-alignment + expansion in one launch:
 *   alpha'[b][i][j] = softmax_i( -sigma (q_j - e[b][i])^2 ), q_j = j for j < mel_len[b] else 0, keys i >= text_len[b] excluded,
 *                     zero outside the text x mel mask   (reconstruct_align_from_aligned_position efficient_tts.py:347-375, :186)
 *   H[b * T2p + j][:] = sum_i alpha'[b][i][j] * V[b * T1p + i][:]   (the expand bmm :190-194; frames j >= mel_len[b] are zero)
 * alpha' is produced in registers as the MFMA A operand (split-bf16: lo*hi + hi*lo + hi*hi, as efts_gemm on split-2 planes)
 * and never stored as an operand plane; V is read as fp32 from its row space (no V^T planes).  Lengths NULL = inference (no
 * masks, :270-274).  Outputs, any combination: alpha_out (the API tensor [B][T1][T2] fp32), y_f32 (row space [B*T2p][ldo]),
 * y (operand plane of format y_split; with y_split 1 an optional remainder plane y_lo).  Rows j >= T2 of the row space are
 * not touched.  T1 <= 256, n % 128 == 0. */
typedef struct efts_expand_args {
    const float* e;          /* [B][T1] aligned positions */
    const int32_t* text_len; /* [B] or NULL */
    const int32_t* mel_len;  /* [B] or NULL */
    float sigma;
    const float* v;          /* value projection, fp32 row space [B * T1p][ldv] */
    int64_t ldv;             /* elements */
    int32_t B, T1, T1p, T2, T2p;
    int32_t n;               /* channels */
    float* alpha_out;        /* [B][T1][T2] or NULL */
    float* y_f32;            /* [B * T2p][ldo] or NULL */
    int64_t ldo;             /* elements */
    void* y;                 /* operand plane (row 0) or NULL */
    void* y_lo;              /* y_split 1 only: bf16 remainder plane or NULL */
    int64_t ldy;             /* bytes, both planes */
    int32_t y_split;
} efts_expand_args;
int efts_expand(const efts_expand_args* a, void* stream);

/* Between the two phases of free-running synthesis (efficient_tts.py:258-270), one launch per batch: e[b][i] = cumulative sum of
 * the durations dur[b * ld + i] (i < T1; efts_cumsum_rows' scan), mel_len[b] = round-half-even(e[b][text_len[b] - 1]), and with
 * method1 == 0 the positions start at 0 (e[b][i] -= dur[b][i], :261-265).  force_delta >= 0 replaces every valid duration by that
 * value (benchmark hook: a synthetic batch then yields a known mel length); < 0: off. */
int efts_duration_positions(const float* dur, int64_t ld, const int32_t* text_len, float force_delta, int32_t method1, float* e,
                            int32_t* mel_len, int32_t B, int32_t T1, void* stream);

/* efts_duration_positions with duration control, one launch per batch (same scan; with every control NULL the results are
 * efts_duration_positions' bit for bit).  Every control may be NULL:
 *   length_scale [B]      multiplies every duration of item b (> 0 and finite);
 *   override_frames [B][ldo]  frames per token: entries >= 0 replace dur (valid tokens only), negative ones keep it; the scale
 *                         applies to replaced entries too.  dur may be NULL when the overrides cover every valid token;
 *   target_frames [B]     after the scan, item b is rescaled so that its last inclusive position E_{len-1} is target_frames[b]
 *                         exactly (>= 1; a zero total duration cannot be rescaled), and mel_len[b] = target_frames[b].
 * e [B][T1] and mel_len [B] as efts_duration_positions (method1 == 0: positions from 0).  frames [B][T1] (optional):
 * frames[b][i] = round(E_i) - round(E_{i-1}) with E the inclusive cumulative (scaled) duration, E_{-1} = 0, round half-even;
 * 0 past text_len, so sum_i frames[b][i] == mel_len[b] (each boundary is rounded from one fp32 value, also across the scan's
 * chunks).  A rejected item (bad scale or target, a total that does not fit an int32, a negative override without dur) gets
 * mel_len[b] = -1 (and frames 0). */
int efts_duration_control(const float* dur, int64_t ld, const int32_t* text_len, const float* length_scale, const float* override_frames,
                          int64_t ldo, const int32_t* target_frames, int32_t method1, float* e, int32_t* mel_len, int32_t* frames,
                          int32_t B, int32_t T1, void* stream);

/* The fp32 -> bf16 rounding of every operand-plane producer in this library (round to nearest even; torch's
 * .to(torch.bfloat16)): mode 0 = as the kernels do it (gfx950's packed conversion instruction), mode 1 = the integer
 * reference form.  y[i] = bf16 bits of x[i].  Exists so that a test can sweep bit patterns through both. */
int efts_bf16_round(const float* x, uint16_t* y, int64_t n, int32_t mode, void* stream);

/* ------------------------------------------------------------------------------------
 * Duration predictor tail (nntts/layers/duration_predictor.py:57-88, layer_norm.py:6-30).
 * efts_layernorm_rows: y = LN_c(x) * gamma + beta (biased variance, eps), times rowmask[row];
 *   writes fp32 (optional) and/or an A operand plane.
 * efts_layernorm_dot: out[row] = dot(LN_c(x[row]), w) + b  (LayerNorm + Linear(c,1) + squeeze);
 *   mode 0: log domain, * rowmask (masked_fill(x_masks, 0), :85-86)
 *   mode 1: inference, max(exp(.) - offset, 0)  (:78-83, to_round=False), * rowmask if given.
 * drop_p > 0 applies the module's Dropout(0.1) after the LayerNorm (:61, train mode): a stateless
 * counter-based mask from (drop_seed, element index), regenerated identically by efts_layernorm_bwd.
 * drop_seed_add (optional, device): one word added to drop_seed when the kernel runs -- the step counter of a training step that
 * is replayed as a hipGraph, where by-value arguments are frozen at capture time.
 * ---------------------------------------------------------------------------------- */
int efts_layernorm_rows(const float* x, const float* gamma, const float* beta, float eps,
                        const float* rowmask, float* f32_out, void* plane, int64_t ld_plane,
                        int32_t rows, int32_t c, int32_t split, float drop_p, uint32_t drop_seed, const uint32_t* drop_seed_add, void* stream);
int efts_layernorm_dot(const float* x, const float* gamma, const float* beta, float eps, const float* w,
                       const float* b, const float* rowmask, int32_t mode, float offset, float* out,
                       int32_t rows, int32_t c, float drop_p, uint32_t drop_seed, const uint32_t* drop_seed_add, void* stream);

/* ------------------------------------------------------------------------------------
 * FastSpeechLoss with use_masking=True (nntts/losses/fastspeech_loss.py:54-67):
 * out[0] = loss, out[1] = mel MSE over valid frames, out[2] = duration L1 over valid tokens.
 * mel_pred: row space [B*T2p][ldm]; speech [B][T2][odim]; dur_pred/log_delta_e row space /
 * [B][T1] resp.  workspace: >= efts_losses_workspace_bytes() bytes.
 * ---------------------------------------------------------------------------------- */
size_t efts_losses_workspace_bytes(void);
int efts_masked_losses(const float* mel_pred, int64_t ldm, const float* speech, const int32_t* mel_len,
                       const float* dur_pred, const float* log_delta_e, const int32_t* text_len,
                       float* out3, void* workspace, int32_t B, int32_t T1, int32_t T1p, int32_t T2,
                       int32_t T2p, int32_t odim, void* stream);
/* The same losses when the mel head's launch already left the squared-error partial sums (efts_gemm_args.sqerr_part, n_part of
 * them): one single-workgroup launch adds them up in index order, takes the duration L1 itself and writes out[0..2] as above. */
int efts_losses_from_parts(const float* sqerr_part, int32_t n_part, const int32_t* mel_len, const float* dur_pred,
                           const float* log_delta_e, const int32_t* text_len, float* out3, int32_t B, int32_t T1,
                           int32_t T1p, int32_t T2, int32_t odim, void* stream);

/* ====================================================================================
 * Training step (backward + optimizer).  The reference backward is torch autograd of the
 * forward ops (loss.backward(), nntts/trainers/efficient_tts_trainer.py:153); these entry
 * points are its hand-written equivalents.  MFMA-shaped gradients (conv/linear dgrad and
 * wgrad, the four products of the alignment block) run through efts_gemm on operand planes
 * produced here.
 * ==================================================================================== */
/* folded weight w[cout][cin][taps] -> dgrad B plane [taps][cin rows][K = cout], taps flipped */
int efts_pack_weight_t(const float* w, void* plane, int64_t ldb, int32_t cout, int32_t cin, int32_t taps,
                       int32_t split, void* stream);
/* Weight preparation of a whole group of equally shaped Conv1d / Linear weights in one call (2 launches): per item
 * efts_pack_weight (plane and/or w_f32_out; either may be NULL) and, with with_t != 0, efts_pack_weight_t into plane_t
 * (NULL = skip the item) from the folded weight.  `items` is an array in DEVICE memory.  scale_ws: n_items * cout
 * floats of device scratch (weight-norm scales); with it, shapes with cout % 64 == 0, cin % 64 == 0, taps <= 5 take
 * the tiled path (one pass over the weights writes both planes); NULL or other shapes: row kernels, which leave the
 * scales in scale_ws too.  Both paths write the same bytes into plane, plane_t and w_f32_out.  PRECONDITION: a
 * weight-normed item (g != NULL) that has a plane_t needs w_f32_out or scale_ws -- the row kernels fold plane_t from
 * the one or the other; with neither they fill the item's plane_t with NaN instead of packing the unfolded weight.
 * With with_t == 0 no plane_t is written on either path.  The reference does this work implicitly per layer and step:
 * the weight_norm hook (efts_modules.py:92-99) in every forward, the transposed operand inside cuDNN's dgrad. */
typedef struct efts_pack_item {
    const float* w;        /* [cout][cin][taps] fp32: weight_v, or the plain weight when g == NULL */
    const float* g;        /* weight-norm gain [cout] or NULL */
    float* w_f32_out;      /* folded fp32 copy [cout][cin][taps] or NULL */
    void* plane;           /* forward B plane [taps][cout][Kp(cin)], row stride ldb, or NULL */
    void* plane_t;         /* transposed + tap-flipped dgrad plane [taps][cin][Kp(cout)], row stride ldb_t, or NULL */
} efts_pack_item;
int efts_pack_weights_grouped(const efts_pack_item* items, int32_t n_items, float* scale_ws, int64_t ldb, int64_t ldb_t,
                              int32_t cout, int32_t cin, int32_t taps, int32_t split, int32_t with_t, void* stream);
/* d loss / d mel_pred (fp32 [B*T2p][odim] and/or operand plane) and d loss / d dur_pred [B*T1p]
 * of FastSpeechLoss(use_masking) (fastspeech_loss.py:54-67); gscale: device scalar or NULL (1). */
int efts_loss_bwd(const float* mel_pred, int64_t ldm, const float* speech, const int32_t* mel_len,
                  const float* dur_pred, const float* log_delta_e, const int32_t* text_len, const float* gscale,
                  float* dmel, void* dmel_plane, int64_t ld_plane, int32_t split, float* ddur, int32_t B, int32_t T1,
                  int32_t T1p, int32_t T2, int32_t T2p, int32_t odim, void* stream);
/* dZ = G * act'(.) * rowmask, bias grad += column sums.  mode 1: residual LeakyReLU layer
 * (sign from y - x); 2: ReLU (sign of y); 3: LeakyReLU without residual (sign of y); 0: identity;
 * 5: LeakyReLU with the plain sign bits efts_resconv5 wrote (`sign_bits`) passed as y (row stride c / 8 bytes);
 * 4: LeakyReLU with the sign words efts_gemm wrote (`sign_mask` of the forward launch) passed as y (row stride c / 8 bytes,
 * c % 128 == 0), x unused.
 * plane (optional): rows of Kp(c) values, the K padding c .. Kp written as zero; ld_plane >= the bytes of Kp values.
 * mode | EFTS_ACT_BWD_BIAS_PARTS: dbias is a [ceil(rows / 64)][c] workspace that receives one column sum per 64-row block
 * (plain stores, overwritten) instead of atomic adds into the gradient; efts_wgrad_reduce_grouped adds them up. */
#define EFTS_ACT_BWD_BIAS_PARTS 16
/* efts_act_bwd with the Dropout mask of the forward launch (efts_gemm_args.drop_p / drop_seed, c = that launch's n) applied too */
int efts_act_bwd_dropout(const float* g, const float* y, const float* x, const float* rowmask, float slope, int32_t mode,
                         float* dz, void* plane, int64_t ld_plane, int32_t split, float* dbias, int32_t rows, int32_t c,
                         float drop_p, uint32_t drop_seed, void* stream);
int efts_act_bwd(const float* g, const float* y, const float* x, const float* rowmask, float slope, int32_t mode,
                 float* dz, void* plane, int64_t ld_plane, int32_t split, float* dbias, int32_t rows, int32_t c,
                 void* stream);
/* The residual layer's non-linearity when it is not (Leaky)ReLU: the reference builds getattr(torch.nn, nonlinear_activation)(**params)
 * into every ResConv1d and into the mel prenet (nntts/layers/efts_modules.py:32-35, nntts/models/efficient_tts.py:76-80).  The contraction then
 * writes the pre-activation z = conv(x) + bias in fp32 (efts_gemm with EFTS_ACT_NONE) and these two elementwise launches do the rest.
 * p0 / p1: the module's scalar parameters, in the order of the comments below (unused ones are ignored). */
#define EFTS_ACTFN_IDENTITY 0
#define EFTS_ACTFN_RELU 1
#define EFTS_ACTFN_LEAKY_RELU 2  /* p0 = negative_slope */
#define EFTS_ACTFN_ELU 3         /* p0 = alpha */
#define EFTS_ACTFN_CELU 4        /* p0 = alpha */
#define EFTS_ACTFN_SELU 5
#define EFTS_ACTFN_GELU 6        /* approximate="none" (erf) */
#define EFTS_ACTFN_GELU_TANH 7   /* approximate="tanh" */
#define EFTS_ACTFN_SILU 8
#define EFTS_ACTFN_MISH 9
#define EFTS_ACTFN_TANH 10
#define EFTS_ACTFN_SIGMOID 11
#define EFTS_ACTFN_SOFTPLUS 12   /* p0 = beta, p1 = threshold */
#define EFTS_ACTFN_HARDTANH 13   /* p0 = min_val, p1 = max_val (ReLU6 = 0, 6) */
#define EFTS_ACTFN_HARDSWISH 14
#define EFTS_ACTFN_HARDSIGMOID 15
#define EFTS_ACTFN_SOFTSIGN 16
#define EFTS_ACTFN_TANHSHRINK 17
#define EFTS_ACTFN_LOGSIGMOID 18
#define EFTS_ACTFN_COUNT 19
/* y = (resid + Dropout(f(z))) * rowmask over [rows][c] fp32 (c % 4 == 0): y_f32 and / or the operand plane (either may be NULL, not both);
 * resid, rowmask may be NULL; Dropout as in the argument block of efts_gemm: drop_p / drop_seed, element index row * c + col */
int efts_act_apply(const float* z, const float* resid, const float* rowmask, int32_t act, float p0, float p1, float* y_f32, void* plane,
                   int64_t ld_plane, int32_t split, int32_t rows, int32_t c, float drop_p, uint32_t drop_seed, void* stream);
/* dZ = G * rowmask * Dropout'(.) * f'(z): dz (fp32) and / or the operand plane; dbias (may be NULL) += column sums of dZ (atomic adds) */
int efts_act_grad(const float* g, const float* z, const float* rowmask, int32_t act, float p0, float p1, float* dz, void* plane,
                  int64_t ld_plane, int32_t split, float* dbias, int32_t rows, int32_t c, float drop_p, uint32_t drop_seed, void* stream);
/* transposed operand planes out_s[ch][t] = x[t + shift0 + s][ch], s = 0..nshift-1 (plane s at
 * plane + s*plane_stride bytes), K = t padded with zeros to kpad: the wgrad operands of all taps
 * from one pass over x */
int efts_pack_t(const float* x, int64_t ldx, void* plane, int64_t ld_plane, int64_t plane_stride, int32_t split,
                int32_t rows, int32_t c, int32_t shift0, int32_t nshift, int32_t kpad, void* stream);
/* Reduction of the transposed-plane path's split-K partials (taps x split-K efts_gemm launches over efts_pack_t planes: the path of shapes
 * the direct kernel's tiles do not fit): dW[co][ci][k] = sum_s part[k][s][co][ci]; with g != NULL also the weight-norm backward
 * (dv -> dw_or_dv, dg) of w = g v / ||v|| */
int efts_wgrad_reduce(const float* part, int32_t nsplit, const float* v, const float* g, float* dw_or_dv, float* dg,
                      int32_t cout, int32_t cin, int32_t taps, void* stream);
/* Direct weight gradients of k5 / k3 convolutions and Linears (taps 5, 3, 1) from the ROW-MAJOR bf16 planes (no transposed copies):
 *   dW[co][ci][k] = sum_t dZ[t][co] * X[t + k - (taps - 1) / 2][ci]      (autograd of the Conv1d in nntts/layers/efts_modules.py:48-51)
 * dz_plane / x_plane: operand planes of the row space, both of format `split` (1 = bf16, 2 = bf16x3 hi/lo) (row 0 pointers; >= 2 zero rows
 * before row 0 and >= 144 after `rows`), cout % 128 == 0, cin % 64 == 0.
 * The weight gradients of up to EFTS_WGRAD_MAX_ITEMS layers (same rows, cout, cin, taps and plane
 * format; e.g. the Conv1d of every ResConv1d of a `ResConvBlock`, nntts/layers/efts_modules.py:77-79 under
 * nntts/trainers/efficient_tts_trainer.py:146) in ONE launch.  The (layer, tile, 64-row step) space is dealt out to `workgroups`
 * workgroups (0: two per CU) as equal contiguous ranges (stream-K); every workgroup leaves one fp32 slab per tile its range touches
 * in `part` (efts_wgrad_grouped_part_bytes() bytes; -1: bad arguments), and efts_wgrad_reduce_grouped -- called with the SAME count, rows, cout, cin,
 * taps, split and workgroups -- adds a tile's slabs in a fixed order, then per layer the weight-norm backward (g != NULL) and the bias
 * gradient dbias[co] += sum_i bias_part[i][co], i < nparts (the workspace efts_act_bwd fills in EFTS_ACT_BWD_BIAS_PARTS mode, or a dgrad
 * launch's act_bwd_bias_part), in a fixed order.  The launch leaves its geometry behind the slabs (the last 64 bytes of `part`); a reduction whose
 * arguments do not match the launch that filled `part` writes NaN into every output instead of a sum over slabs that were never written. */
#define EFTS_WGRAD_MAX_ITEMS 8
typedef struct efts_wgrad_item {
    const void* dz_plane;   /* operand plane of dZ, row 0 */
    int64_t ldz;
    const void* x_plane;    /* operand plane of the layer's input, row 0 */
    int64_t ldx;
    const float* v;         /* weight_v [cout][cin][taps] (with g) or NULL */
    const float* g;         /* weight_g [cout] or NULL: no weight-norm backward, dw_or_dv receives dW */
    float* dw_or_dv;        /* [cout][cin][taps] */
    float* dg;              /* [cout] or NULL */
    const float* bias_part; /* [nparts][cout] column sums efts_act_bwd left (EFTS_ACT_BWD_BIAS_PARTS), or NULL */
    float* dbias;           /* [cout], += */
    int32_t nparts;
    int32_t reserved;
} efts_wgrad_item;
int64_t efts_wgrad_grouped_part_bytes(int32_t count, int32_t rows, int32_t cout, int32_t cin, int32_t taps, int32_t split,
                                      int32_t workgroups);
int efts_wgrad_tn_grouped(const efts_wgrad_item* items, int32_t count, float* part, int32_t rows, int32_t cout, int32_t cin,
                          int32_t taps, int32_t split, int32_t workgroups, void* stream);
int efts_wgrad_reduce_grouped(const efts_wgrad_item* items, int32_t count, const float* part, int32_t rows, int32_t cout,
                              int32_t cin, int32_t taps, int32_t split, int32_t workgroups, void* stream);
/* backward of [ReLU ->] LayerNorm [-> Linear(c,1)] (duration_predictor.py:57-77); accumulates
 * dgamma, dbeta, conv-bias grad (dbias), and with ddur != NULL the Linear's dw, db. */
int efts_layernorm_bwd(const float* x, const float* gamma, const float* beta, float eps, const float* dy,
                       const float* ddur, const float* w, const float* rowmask, float* dz, void* plane,
                       int64_t ld_plane, int32_t split, float* dgamma, float* dbeta, float* dbias, float* dw, float* db,
                       int32_t rows, int32_t c, float drop_p, uint32_t drop_seed, const uint32_t* drop_seed_add, void* stream);
/* alignment block backward (efficient_tts.py:287-398 under autograd).  Every entry point refuses non-positive B, T1, T2 with
 * EFTS_ESHAPE before any launch.
 * efts_alpha_bwd: r_ws[b][j] = sum_i alpha'_ij dalpha_ij, de[b][i] (0 at i >= text_len).  ralpha is the masked alpha' of the forward
 *   (0 outside text x mel); dalpha must be finite there (the caller's product with the masked dH leaves 0). */
int efts_alpha_bwd(const float* ralpha, const float* dalpha, const float* e, const int32_t* text_len,
                   const int32_t* mel_len, float sigma, float* r_ws /* [B*T2] */, float* de, int32_t B, int32_t T1,
                   int32_t T2, void* stream);
/* efts_e_bwd: dpi[b][j] (0 at j >= mel_len).  One item's e, de and softmax statistics live in 4 * T1 floats of LDS: EFTS_ESHAPE when they
 *   exceed the 64 KiB of the launch (T1 > 4096). */
int efts_e_bwd(const float* imv, const float* e, const float* de, const int32_t* text_len, const int32_t* mel_len,
               float sigma_e, float* stats_ws /* [2*B*T1] */, float* dpi, int32_t B, int32_t T1, int32_t T2,
               void* stream);
int efts_imv_bwd(const float* soft_idx, const float* imv, const float* dpi, const int32_t* text_len,
                 const int32_t* mel_len, float* dsoft_idx, int32_t B, int32_t T2, void* stream);
/* efts_attn_bwd: dscores [B*T2][ldd] (columns < T1) and its bf16x3 A plane, rows (b*T2p + j), K = i padded with zeros to a multiple of 32.
 *   EFTS_ESHAPE for ld < T1, ldd < T1, T2p < T2 or ld_plane < ceil(T1 / 32) * 128. */
int efts_attn_bwd(const float* scores, int64_t ld, const float* soft_idx, const float* dsoft_idx,
                  const int32_t* text_len, const int32_t* mel_len, float* dscores, int64_t ldd, void* plane,
                  int64_t ld_plane, int32_t B, int32_t T1, int32_t T2, int32_t T2p, void* stream);
/* efts_embed_bwd: dtable[ids[b][t]] += g[b*Tp + t] for t < T (ids [B][T] contiguous, g in the padded row space; ids clamped to the table).
 *   EFTS_ESHAPE for non-positive B, T, c, num_symbols or Tp < T. */
int efts_embed_bwd(const int64_t* ids, const float* g, float* dtable, int32_t B, int32_t T, int32_t Tp, int32_t c,
                   int32_t num_symbols, void* stream);
/* clip_grad_norm_ + torch.optim.Adam(amsgrad=True, coupled weight decay) on flat fp32 buffers
 * (trainer.py:154-158; YAML :34-40).  efts_sumsq ACCUMULATES sum(g^2) into *out1 (zero it first) with a
 * deterministic two-stage reduction (workspace >= efts_sumsq_workspace_bytes());
 * efts_adam_amsgrad scales g by gscale * min(1, max_norm / (gscale*sqrt(sumsq) + 1e-6)). */
size_t efts_sumsq_workspace_bytes(void);
int efts_sumsq(const float* g, int64_t n, float* out1, void* workspace, void* stream);
/* x[0..n) *= *scale (device scalar), skipped on the device when *scale == 1: the `grad_output` factor of
 * loss.backward() on the flat gradient buffer (torch autograd semantics of nntts/trainers/efficient_tts_trainer.py:150). */
int efts_scale_unless_one(float* x, int64_t n, const float* scale, void* stream);
int efts_adam_amsgrad(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, const float* sumsq,
                      float max_norm, float gscale, float lr, float beta1, float beta2, float eps, float weight_decay,
                      int32_t step, void* stream);
/* The same update with its per-step scalars in DEVICE memory -- hyper = {lr, 1 - beta1^step, sqrt(1 - beta2^step)}, as
 * efts_adam_hyper (host) computes them, bit for bit what efts_adam_amsgrad derives from its by-value arguments -- so that a whole
 * training step (nntts/trainers/efficient_tts_trainer.py:139-160) can be captured once and replayed as a hipGraph: the host only
 * refreshes the words in front of every replay (efts_store_words: up to 8 32-bit words passed by value, stream-ordered; the same
 * call carries the dropout step word of efts_layernorm_rows / _dot / _bwd `drop_seed_add`). */
int efts_adam_hyper(float lr, float beta1, float beta2, int32_t step, float* out3 /* host */);
int efts_adam_amsgrad_dev(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, const float* sumsq,
                          float max_norm, float gscale, const float* hyper, float beta1, float beta2, float eps,
                          float weight_decay, void* stream);
int efts_store_words(uint32_t* dst /* device */, const uint32_t* words /* host */, int32_t n, void* stream);

/* The rest of the Adam family behind the reference's optimizer registry (nntts/optimizers/__init__.py: torch.optim + radam.py), same
 * flat buffers and the same clip -- coef = gscale * min(1, max_norm / (gscale*sqrt(sumsq) + 1e-6)), gg = coef * g -- in ONE launch:
 *   EFTS_OPTIM_ADAM   torch.optim.Adam : gg += wd p;  m = b1 m + (1-b1) gg;  v = b2 v + (1-b2) gg^2;  vh = amsgrad ? (vmax = max(vmax, v)) : v;
 *                                        p -= lr / (1 - b1^t) * m / (sqrt(vh) / sqrt(1 - b2^t) + eps)
 *   EFTS_OPTIM_ADAMW  torch.optim.AdamW: p *= 1 - lr wd first, no wd in gg, the rest as ADAM
 *   EFTS_OPTIM_RADAM  nntts/optimizers/radam.py (NOT torch.optim.RAdam: threshold, eps placement and decay differ):
 *                                        v, m from gg;  p *= 1 - wd lr;  N = N_max - 2 t b2^t / (1 - b2^t), N_max = 2 / (1 - b2) - 1;
 *                                        N >= 5: p -= lr s m / (sqrt(v) + eps), s = sqrt((1 - b2^t)(N - 4)/(N_max - 4) (N - 2)/N N_max/(N_max - 2)) / (1 - b1^t)
 *                                        else  : p -= lr m / (1 - b1^t).  No amsgrad form.
 * Elementwise fp32; everything that depends on the step number or the learning rate is four words computed on the host in double,
 *   ADAM / ADAMW {lr / (1 - b1^t), sqrt(1 - b2^t), 1 (ADAM) or 1 - lr wd (ADAMW), 0}      RADAM {lr s, 1, 1 - wd lr, N >= 5 ? 1 : 0}
 * taken from lr / step by value, or, with hyper != NULL, read from DEVICE memory (lr and step are then ignored): efts_optim_hyper
 * returns exactly the words the by-value path derives, so a hipGraph replay and an eager step give the same bits (as efts_adam_hyper
 * for efts_adam_amsgrad_dev).  The scalars are doubles so that (float)(1 - beta) is rounded once, as torch's fp32 kernels receive it.
 * amsgrad == 0: vmax is neither read nor written (may be NULL).  Two runs give the same bits (no atomics).
 * EFTS_EINVAL: NULL p / g / m / v / out4, vmax NULL with amsgrad, n <= 0, step < 1 (by value), unknown algo, RADAM with amsgrad, a beta outside
 * [0, 1).  EFTS_EALIGN: p, g, m, v, vmax not 16-byte aligned. */
#define EFTS_OPTIM_ADAM 0
#define EFTS_OPTIM_ADAMW 1
#define EFTS_OPTIM_RADAM 2
typedef struct efts_optim_args {
    float* p;               /* [n] parameters, updated in place */
    const float* g;         /* [n] gradients */
    float* m;               /* [n] exp_avg */
    float* v;               /* [n] exp_avg_sq */
    float* vmax;            /* [n] max_exp_avg_sq, amsgrad only (NULL otherwise) */
    int64_t n;
    const float* sumsq;     /* device: sum(g^2) (efts_sumsq), or NULL: no clip */
    float max_norm;         /* <= 0: no clip */
    float gscale;
    int32_t algo;           /* EFTS_OPTIM_* */
    int32_t amsgrad;
    double lr, beta1, beta2, eps, weight_decay;
    int32_t step;           /* >= 1; by-value path only */
    int32_t reserved;
    const float* hyper;     /* device: the four words of efts_optim_hyper, or NULL: derive them from lr / step */
} efts_optim_args;
int efts_optim_step(const efts_optim_args* a, void* stream);
int efts_optim_hyper(int32_t algo, double lr, double beta1, double beta2, double weight_decay, int32_t step, float* out4 /* host */);

/* The exponential moving average of the parameters, kept beside the optimizer state on the same flat fp32 buffer, as a launch of its own
 * behind the optimizer's (efts_optim_args, efts_optim_step and efts_adam_amsgrad are untouched by it):
 *   efts_ema_update : ema[i] = fmaf(w, p[i] - ema[i], ema[i]) for i < n, w = one_minus_decay.  In roundings: d = fl(p - e), one fp32
 *                     subtraction; e' = fl(w d + e), one fused multiply-add, rounded once.  So |e' - exact| <= 2^-24 |p - e| + 2^-24 |e'|
 *                     <= 2^-23 (|p| + |e|) for w in (0, 1).  The two ends are defined by what they mean, not by the formula: w == 0 writes
 *                     nothing (ema stays bit for bit, a -0 included), w == 1 stores p itself (fl(fl(p - e) + e) is not p where |p| is far
 *                     below |e|: the subtraction has already lost p).  3 words per element (p, ema read; ema written), 16-byte
 *                     accesses, 256-thread blocks, at most 2048 blocks that grid-stride, a scalar tail for n % 4; no atomics: two runs give
 *                     the same bits.  w travels by value, the launch can be captured.
 *   efts_ema_hyper  : the ONE definition of the per-update word, on the host in double, rounded to fp32 once:
 *                       d = warmup ? min(decay, (1 + updates) / (10 + updates)) : decay;    out1[0] = (float)(1.0 - d)
 *                     `updates`: the updates already made (0 for the first).  With warm-up the first update takes 9/10 of p, and the ramp
 *                     crosses decay = 0.999 between updates 8990 and 8991.
 * EFTS_EINVAL: NULL ema / p / out1, n <= 0, one_minus_decay outside [0, 1] (NaN included), decay outside [0, 1), updates < 0.
 * EFTS_EALIGN: ema or p not 16-byte aligned. */
int efts_ema_hyper(double decay, int32_t warmup, int64_t updates, float* out1 /* host */);
int efts_ema_update(float* ema, const float* p, int64_t n, float one_minus_decay, void* stream);

/* ------------------------------------------------------------------------------------
 * Log-mel front-end: the data format right before the path.
 * Replaces nntts/datasets/meldataset.py:49-82 (mel_spectrogram, computed per item on CPU dataloader
 * workers by TextMelLoader.get_mel, taco2_data.py:66-76) and the mel half of TextMelCollate
 * (taco2_data.py:122-139) with a batched device pipeline:
 *   efts_frame_pack : audio fp32 [B][ld_audio] in [-1,1], per-item sample counts `lengths` ->
 *                     A operand plane rows (b*Tp + t), K = n_fft: frame t of item b =
 *                     reflect_pad(audio_b, (n_fft-hop)/2)[t*hop + k] * window[k]  (:69-73);
 *                     frames past L_b / hop and gap rows are zero.
 *   efts_gemm       : taps 1, against a B plane of the real DFT (rows 0..n_bins-1 = cos, rows
 *                     n_bins..2*n_bins-1 = -sin), fp32 output [rows][ld_spec >= 2*n_bins].
 *   efts_logmel     : out[b][t][m] = log(max(sum_k basis[m][k] * sqrt(re^2+im^2+1e-9), 1e-5)) for
 *                     t < frames[b], else 0 (:75-78, :27-28; zero padding after the log as the
 *                     collate does).  basis fp32 [n_mels][n_bins]; ranges int32 [n_mels][2] = the
 *                     [lo, hi) span of non-zero basis entries of each filter.  out is the contiguous
 *                     [B][T][n_mels] tensor EfficientTTSCNN.forward takes as `speech`.
 * ---------------------------------------------------------------------------------- */
int efts_frame_pack(const float* audio, int64_t ld_audio, const int32_t* lengths, const float* window, void* plane,
                    int64_t ld_plane, int32_t B, int32_t T, int32_t Tp, int32_t n_fft, int32_t hop, int32_t split,
                    void* stream);
int efts_logmel(const float* spec, int64_t ld_spec, const float* basis, const int32_t* ranges, const int32_t* frames,
                float* out, int32_t B, int32_t T, int32_t Tp, int32_t n_bins, int32_t n_mels, void* stream);
/* The same pipeline with the DFT split by decimation in time (round 6): `radix` interleaved sub-sequences x_p[j] = x[radix j + p] of
 * M = n_fft / radix samples each.
 *   efts_frame_pack_dit : as efts_frame_pack, but column p * M + j of a row holds sample radix * j + p of the frame, so that ONE batched
 *                         efts_gemm (batch = radix, a_batch_stride = the bytes of M columns, nchunk = the chunks of M columns, n = M,
 *                         out_batch_stride = M) against the B plane of the real M-point DFT -- rows 0 .. M/2: cos(2 pi g j / M), rows
 *                         M/2 + g, g = 1 .. M/2 - 1: -sin(2 pi g j / M) -- leaves, per row, `radix` blocks [re Y_p[0 .. M/2] | im Y_p[1 .. M/2 - 1]]:
 *                         radix times fewer FLOPs than the dense n_fft-point product.
 *   efts_logmel_dit     : X[f] = sum_p W^(p f) Y_p[f mod M] (Y_p[M - g] = conj Y_p[g]) in front of the magnitude, then as efts_logmel.
 *                         twiddle: fp32 [radix][n_bins][2] = (cos, sin)(2 pi p f / n_fft).  spec rows hold n_fft floats. */
int efts_frame_pack_dit(const float* audio, int64_t ld_audio, const int32_t* lengths, const float* window, void* plane,
                        int64_t ld_plane, int32_t B, int32_t T, int32_t Tp, int32_t n_fft, int32_t hop, int32_t split,
                        int32_t radix, void* stream);
int efts_logmel_dit(const float* spec, int64_t ld_spec, const float* basis, const int32_t* ranges, const int32_t* frames,
                    const float* twiddle, float* out, int32_t B, int32_t T, int32_t Tp, int32_t n_bins, int32_t n_mels, int32_t radix,
                    void* stream);

/* The whole front-end as ONE launch (round 6; n_fft 1024, hop 256, n_mels <= 80: the reference's configuration): audio in, log-mels out, the
 * STFT as an fp32 FFT in registers and LDS -- one wave per pair of neighbouring frames (two real frames = one complex 1024-point FFT, taken apart
 * by conjugate symmetry), no operand plane and no spectrum in memory.  Arguments as efts_frame_pack (audio, lengths, window) and efts_logmel
 * (basis, ranges, out); the frame count of item b is lengths[b] / hop; out[b][t][:] = 0 for t past it.  Other configurations: the three-launch
 * pipeline above. */
int efts_logmel_fft(const float* audio, int64_t ld_audio, const int32_t* lengths, const float* window, const float* basis,
                    const int32_t* ranges, float* out, int32_t B, int32_t T, int32_t n_fft, int32_t hop, int32_t n_mels, void* stream);
/* ... straight from int16 PCM, as TextMelLoader.get_mel reads a waveform (taco2_data.py:66-76): every sample is multiplied by pcm_scale
 * (1 / max_wav_value = 1 / 32768: exact in fp32) at the load -- the same bits as converting the batch first, without the conversion pass. */
int efts_logmel_fft_pcm16(const int16_t* audio, int64_t ld_audio, float pcm_scale, const int32_t* lengths, const float* window, const float* basis,
                          const int32_t* ranges, float* out, int32_t B, int32_t T, int32_t n_fft, int32_t hop, int32_t n_mels, void* stream);

/* ------------------------------------------------------------------------------------
 * HiFi-GAN generator (nntts/vocoders/hifigan_model.py:95-136): every Conv1d /
 * ConvTranspose1d of it is an efts_gemm call (dilated taps 3 / 7 / 11, `plane_act` for the pre-activation
 * residual blocks, a stride-u transposed convolution = a 2-tap convolution with u * cout output columns,
 * EFTS_ACT_TANH for the output layer).  The one remaining elementwise step:
 * efts_mean_act_rows: m = (a + b + c) * scale (b, c optional); out (optional) = m; plane (optional) =
 *   operand plane of LeakyReLU(m, slope): the multi-receptive-field mean `xs / num_kernels` (:123-131)
 *   and the activation its consumer applies to its input.  a, b, c: fp32 [rows][ld], c % 4 == 0.
 * ---------------------------------------------------------------------------------- */
int efts_mean_act_rows(const float* a, const float* b, const float* c3, int64_t ld, float scale, float slope, float* out,
                       int64_t ldo, void* plane, int64_t ld_plane, int32_t split, int32_t rows, int32_t c, void* stream);

/* ------------------------------------------------------------------------------------
 * Griffin-Lim vocoder (Griffin & Lim 1984, momentum of Perraudin et al. 2013) for the analysis configuration of efts_logmel_fft:
 * n_fft 1024, hop 256, periodic Hann `window` [1024], 384 samples of padding per side, frames not centred -- frame t starts at
 * padded sample 256 t, and T frames describe a padded signal y_pad of 256 T + 768 samples.  fp32 throughout, the transforms as the
 * front-end's register / LDS FFT (two real frames per complex transform).
 *   spec, spec_prev, spec_out : [B][T][513] complex (re, im interleaved), 8-byte aligned (EFTS_EALIGN otherwise)
 *   mag                       : [B][T][513] target magnitudes
 *   wframes                   : [B][T][1024] windowed time frames
 *   frames                    : [B] frame counts (clamped to 0 .. T); frames at or beyond an item's count are neither read nor
 *                               written and add nothing to the overlap-add or to the window sum
 * efts_gl_init        : spec = mag e^(i phi), spec_prev = 0.  mode 0: phi = 0; mode 1: phi = 2 pi u, u = (hash >> 8) / 2^24 with the
 *                       counter-based hash of the Dropout masks over (seed, t * 513 + f) -- the same for every item of a batch.
 * efts_gl_synthesis   : wframes[b][t] = window * irfft(spec[b][t]) (the imaginary parts of the DC and Nyquist bins are dropped).
 * efts_gl_analysis    : y_pad[p] = (sum over the frames t' that cover p, oldest first, of wframes[b][t'][p - 256 t']) / max(sum of
 *                       their window^2, 1e-8) -- a gather, never stored -- or, when `signal` is given instead of `wframes`,
 *                       signal[b * ld_signal + p] (ld_signal >= 256 T + 768);  Y = rfft(window * y_pad[256 t ..]);
 *                       C = Y + momentum (Y - spec_prev), spec_out = mag C / max(|C|, 1e-8), spec_prev = Y.
 *                       mag = spec_prev = NULL: the plain analysis, spec_out = Y.  momentum in [0, 1).
 * efts_gl_overlap_add : out[b * ld_out + s] = y_pad[start + s], s < n_out, zero at and beyond 256 frames[b] + 768 - 2 start samples
 *                       (start 384, n_out 256 T: the audio the frames describe; start 0, n_out 256 T + 768: the padded signal).
 * Two runs give the same bits (no atomics).  EFTS_EINVAL / EFTS_ESHAPE / EFTS_EALIGN before any launch; n_fft / hop other than 1024 / 256:
 * EFTS_ESHAPE.
 * ---------------------------------------------------------------------------------- */
int efts_gl_init(const float* mag, float* spec, float* spec_prev, int32_t B, int32_t T, int32_t mode, uint32_t seed, void* stream);
int efts_gl_synthesis(const float* spec, const int32_t* frames, const float* window, float* wframes, int32_t B, int32_t T,
                      int32_t n_fft, int32_t hop, void* stream);
int efts_gl_analysis(const float* wframes, const float* signal, int64_t ld_signal, const int32_t* frames, const float* window,
                     const float* mag, float* spec_prev, float* spec_out, float momentum, int32_t B, int32_t T, int32_t n_fft,
                     int32_t hop, void* stream);
int efts_gl_overlap_add(const float* wframes, const int32_t* frames, const float* window, float* out, int64_t ld_out, int32_t start,
                        int32_t n_out, int32_t B, int32_t T, int32_t n_fft, int32_t hop, void* stream);

/* ------------------------------------------------------------------------------------
 * Sample-rate conversion between integer rates src and dst: a band-limited windowed-sinc interpolator (Kaiser window) in polyphase form.
 * With g = gcd(src, dst), L = dst / g, M = src / g, fc = rolloff * min(1, dst / src), W = ceil(Z / fc), K = 2 W + 1 and, for tau in source
 * samples and u = fc tau,  h(tau) = fc sinc(u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta) for |u| < Z, 0 otherwise (sinc(u) = sin(pi u) / (pi u)):
 *   table : fp32 [L][K], table[p][kk] = h(p / L - (kk - W)), built by the caller (float64, once per rate pair; at most 4 MiB;
 *           efficient_tts_amd/resample.py: Z 64, beta 14.77, rolloff 0.9476 ("best") or Z 16, beta 8.555, rolloff 0.85 ("fast"))
 *   out[b * ld_out + n] = sum over kk = 0 .. K-1, in one fixed order, of x_b[i0 - W + kk] * table[p][kk],  i0 = floor(n M / L), p = (n M) mod L
 *           (positions in 64 bits), for n < out_len(b) = (lengths[b] * L + M - 1) / M;  0 for out_len(b) <= n < ld_out: a padded batch.
 *           x_b[i] = in[b * ld_in + i] for 0 <= i < lengths[b] (clamped to 0 .. ld_in) and 0 otherwise: nothing outside an item's samples is read.
 *   out_lengths[b] = min(out_len(b), ld_out), written by the kernel.
 * fp32 accumulation, no atomics: two runs give the same bits, and an item gives the same bits in any batch as alone.
 * efts_resample_pcm16: the same kernel on int16 PCM, every sample multiplied by pcm_scale (1 / 32768: exact) at the load, as efts_logmel_fft_pcm16.
 * EFTS_EINVAL: null pointer, non-positive or non-coprime L / M, W <= 0.  EFTS_ESHAPE: B outside 1 .. 65535, ld_in / ld_out outside 1 .. 2^31,
 * a table above 4 MiB, or a rate ratio so steep that the input window of 512 outputs (511 M / L + K samples) does not fit 64 KiB of LDS.
 * ---------------------------------------------------------------------------------- */
int efts_resample(const float* in, int64_t ld_in, const int32_t* lengths, const float* table, int32_t L, int32_t M, int32_t W, float* out,
                  int64_t ld_out, int32_t* out_lengths, int32_t B, void* stream);
int efts_resample_pcm16(const int16_t* in, int64_t ld_in, float pcm_scale, const int32_t* lengths, const float* table, int32_t L, int32_t M,
                        int32_t W, float* out, int64_t ld_out, int32_t* out_lengths, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * Scoring synthesised speech against a recording: mel-cepstra, and the cost and length of the dynamic-time-warping path between two
 * sequences of them (efficient_tts_amd/score.py turns the two into mel-cepstral distortion).  fp32, no atomics, one workgroup per item or
 * pair and one fixed order of every sum: an item gives the same bits alone, in any batch and in any run.
 *
 * efts_mel_cepstrum: out[b][t][k] = sum over n = 0 .. n_mels - 1, in this order, of table[k][n] * mel[b * item_stride + t * ld + n] for
 *   t < lengths[b] (clamped to 0 .. T), and 0 for lengths[b] <= t < T; rows at or beyond an item's length are not read.  out is dense
 *   [B][T][n_coef]; table [n_coef][n_mels] is built by the caller (efficient_tts_amd/score.py: rows 1 .. n_coef of the orthonormal DCT-II,
 *   sqrt(2 / N) cos(pi k (n + 1/2) / N), float64 rounded once to fp32; row 0 -- loudness -- is left out).
 *   EFTS_EINVAL: null pointer.  EFTS_ESHAPE: n_mels outside 1 .. 128, n_coef outside 1 .. 32, B outside 1 .. 65535, T < 1, ld < n_mels.
 *
 * efts_dtw: x [B][Tx][D] and y [B][Ty][D] with row strides ldx, ldy and item strides (all in floats); item b has x_lengths[b] and
 *   y_lengths[b] rows (clamped to Tx, Ty), rows beyond them are never read.  With the local cost d(i, j) = sqrt(sum over k = 0 .. D - 1,
 *   in this order and fused, of (x_i[k] - y_j[k])^2), the square root correctly rounded:
 *     A(0, 0) = d(0, 0), L(0, 0) = 1;   A(i, j) = d(i, j) + A(p), L(i, j) = 1 + L(p), p the cheapest existing predecessor among
 *     (i-1, j-1), (i-1, j), (i, j-1), tried in this order, a later one replacing an earlier one only when strictly smaller;
 *     cost[b] = A(last row, last column), path_len[b] = L(last row, last column).
 *   An item with a length below 1 gets cost NaN and path_len 0 and nothing of it is read.  No cost matrix exists in memory: a band of
 *   1024 rows advances as an anti-diagonal wavefront that lives in registers and LDS.
 *   EFTS_EINVAL: null pointer.  EFTS_ESHAPE: D outside 1 .. 32, Tx or Ty outside 1 .. EFTS_DTW_MAX_FRAMES, B outside 1 .. 65535, a row
 *   stride below D; nothing is launched.
 * ---------------------------------------------------------------------------------- */
#define EFTS_DTW_MAX_FRAMES 8192
int efts_mel_cepstrum(const float* mel, int64_t ld, int64_t item_stride, const int32_t* lengths, const float* table, float* out, int32_t B,
                      int32_t T, int32_t n_mels, int32_t n_coef, void* stream);
int efts_dtw(const float* x, int64_t ldx, int64_t x_item_stride, const int32_t* x_lengths, int32_t Tx, const float* y, int64_t ldy,
             int64_t y_item_stride, const int32_t* y_lengths, int32_t Ty, int32_t D, float* cost, int32_t* path_len, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * The warping path itself, and the F0 error read along it.
 *
 * efts_dtw_path: the recurrence, tie rule, limits and error codes of efts_dtw (the same kernel body); cost and path_len are bit-identical
 *   to efts_dtw's on the same input.  In addition
 *     path : int32 [B][Tx + Ty - 1][2], 8-byte aligned.  path[b][k] = (i, j), the k-th cell of the chosen path in FORWARD order:
 *            path[b][0] = (0, 0), path[b][path_len[b] - 1] = (x_lengths[b] - 1, y_lengths[b] - 1), every step one of (1, 1), (1, 0), (0, 1).
 *            Rows at and beyond path_len[b] are left untouched; an item with a length below 1 gets cost NaN, path_len 0 and no path.
 *     workspace : device memory, 16-byte aligned, B times the per-pair size that the workspace-size entry below returns for the same
 *            (Tx, Ty); workspace_bytes is what the caller holds.  The forward pass records which predecessor won at every cell -- 2 bits,
 *            a lane's four rows at one column are one byte, laid out by (band of 1024 rows, wavefront step, lane) so that one step
 *            stores 256 contiguous bytes; the per-pair size is ceil(Tx / 1024) (Ty + 255) 256 bytes.  The back-trace runs in the same
 *            launch behind a workgroup barrier and reads the record through LDS, 64 steps at a time.  Contents afterwards: unspecified.
 *   EFTS_EINVAL: null pointer.  EFTS_ESHAPE: as efts_dtw, or a workspace smaller than B pairs need.  EFTS_EALIGN: workspace or path misaligned.
 * The workspace-size entry returns that per-pair size in bytes, 0 when Tx or Ty lies outside 1 .. EFTS_DTW_MAX_FRAMES; it is monotone in both.
 *
 * efts_f0_path_error: f0_a [B][Ta] and f0_b [B][Tb] (row strides lda, ldb in floats; a value > 0 is a voiced frame's F0 in Hz, anything else
 *   unvoiced), path as efts_dtw_path writes it with path_item_stride cells per item, path_len [B] (clamped to 0 .. path_item_stride).
 *   Over the cells (i, j) = path[b][k], k < path_len[b]:
 *     voiced_pairs[b]  = cells with f0_a[b][i] > 0 and f0_b[b][j] > 0
 *     f0_rmse_cents[b] = sqrt(mean over those cells of (1200 log2(f0_a[b][i] / f0_b[b][j]))^2); NaN when voiced_pairs[b] == 0
 *     vuv_error[b]     = cells whose two sides differ in voicing / path_len[b]; NaN when path_len[b] == 0
 *   A cell that points outside a contour counts as unvoiced on that side and nothing is read for it.  One workgroup per item: lane t sums
 *   cells t, t + 256, ... in order, the 256 partial sums are added in one fixed tree.
 *   EFTS_EINVAL: null pointer.  EFTS_ESHAPE: B, Ta or Tb < 1, a row stride below its T, path_item_stride < 1.  EFTS_EALIGN: path misaligned.
 * ---------------------------------------------------------------------------------- */
int64_t efts_dtw_path_workspace_bytes(int32_t Tx, int32_t Ty);
int efts_dtw_path(const float* x, int64_t ldx, int64_t x_item_stride, const int32_t* x_lengths, int32_t Tx, const float* y, int64_t ldy,
                  int64_t y_item_stride, const int32_t* y_lengths, int32_t Ty, int32_t D, float* cost, int32_t* path_len, int32_t* path,
                  void* workspace, int64_t workspace_bytes, int32_t B, void* stream);
int efts_f0_path_error(const float* f0_a, int64_t lda, int32_t Ta, const float* f0_b, int64_t ldb, int32_t Tb, const int32_t* path,
                       int64_t path_item_stride, const int32_t* path_len, float* f0_rmse_cents, float* vuv_error, int32_t* voiced_pairs, int32_t B,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * Pitch tracking: YIN (de Cheveigne & Kawahara 2002) on the frame grid of efts_logmel_fft, so that f0[b][t] belongs to mel[b][t].
 *   audio   : [B][ld] fp32 in [-1, 1]; the pcm16 entry takes int16 PCM and multiplies every sample by pcm_scale at the load
 *   lengths : [B] samples per item (clamped to 0 .. ld).  Item b has frames(b) = lengths[b] / hop frames when lengths[b] > pad, else none
 *   framing : pad = (n_fft - hop) / 2; sample s of frame t is audio index t hop - pad + s, s = 0 .. n_fft - 1, and an index outside
 *             [0, lengths[b]) is reflected: i < 0 -> -i, i >= lengths[b] -> 2 (lengths[b] - 1) - i.  Nothing outside an item's samples is read.
 * Per frame x[0 .. n_fft - 1], with W = n_fft / 2, tau_min = floor(sampling_rate / fmax), tau_max = floor(sampling_rate / fmin) (in double):
 *   d(tau)  = sum over j = 0 .. W - 1, ascending and fused, of (x[j] - x[j + tau])^2,  tau = 1 .. tau_max  (the direct form: the
 *             energy-plus-autocorrelation form cancels in fp32 on periodic frames)
 *   d'(tau) = d(tau) tau / (d(1) + .. + d(tau)), and 1 where that running sum is 0; d'(0) = 1.  The running sum is taken in one fixed order:
 *             lane l of a wave owns the lags l c + 1 .. l c + c, c = ceil(tau_max / 64); the 64 lane totals are scanned, and every lane adds
 *             its lags in ascending order to the total in front of it.
 *   decision: the smallest tau in [tau_min, tau_max - 1] with d'(tau) < threshold; then tau advances while tau + 1 <= tau_max - 1 and
 *             d'(tau + 1) < d'(tau); with s0, s1, s2 = d'(tau - 1), d'(tau), d'(tau + 1): den = (s0 - s1) + (s2 - s1),
 *             shift = 0.5 (s0 - s2) / den clamped to [-1, 1] (0 when den == 0), f0 = sampling_rate / (tau + shift), aperiodicity = s1.
 *             No such tau: the frame is unvoiced, f0 = 0 and aperiodicity = the smallest d' over [tau_min, tau_max - 1].
 *   f0, aperiodicity : [B][T] fp32; 0 for frames at or beyond frames(b)
 *   cmnd    : optional (NULL: not written) [B][T][tau_max + 1], every d'(tau), tau = 0 .. tau_max; 0 for frames at or beyond frames(b)
 * fp32, no atomics: an item gives the same bits alone, in any batch position and in any run.
 * EFTS_EINVAL: null pointer (cmnd excepted).  EFTS_ESHAPE, nothing launched: n_fft other than 512, 1024, 2048; hop outside 1 .. n_fft or
 * n_fft - hop odd; tau_min < 2; tau_max > W (fmin too low for the window); tau_min >= tau_max - 1; fmin, fmax or threshold not positive;
 * B outside 1 .. 65535, T < 1, ld outside 1 .. 2^31 - 1.
 * ---------------------------------------------------------------------------------- */
int efts_yin(const float* audio, int64_t ld, const int32_t* lengths, float* f0, float* aperiodicity, float* cmnd, int32_t B, int32_t T,
             int32_t n_fft, int32_t hop, int32_t sampling_rate, float fmin, float fmax, float threshold, void* stream);
int efts_yin_pcm16(const int16_t* audio, int64_t ld, float pcm_scale, const int32_t* lengths, float* f0, float* aperiodicity, float* cmnd, int32_t B,
                   int32_t T, int32_t n_fft, int32_t hop, int32_t sampling_rate, float fmin, float fmax, float threshold, void* stream);

/* ------------------------------------------------------------------------------------
 * Smoothing the pitch across frames: the cheapest path (Viterbi) over the lags of every frame, on the d' that efts_yin writes.  All costs
 * are integers in Q16 and the recurrence is integer-only, so the path has exactly one right answer: a restatement in 64-bit integers
 * reproduces it bit for bit (tests/viterbi_reference.py does), and no tolerance applies to it.
 *   cmnd    : fp32, d'(tau) of item b, frame t at cmnd[b * item_stride + t * frame_stride + tau], tau = 0 .. tau_max (strides in floats, the
 *             lag is the unit-stride axis); only frames below the item's count are read
 *   frames  : [B]; item b has n = frames[b] clamped to 0 .. T frames.  n = 0 is legal.
 *   ranges  : 2 <= tau_min < tau_max - 1, tau_max <= EFTS_VITERBI_MAX_LAG
 *   states  : S = tau_max - tau_min voiced states, state s is the lag k = tau_min + s (lags tau_min .. tau_max - 1); state S is unvoiced
 * Fixed point, Q = 65536:
 *   lg      : int32 [tau_max + 1], lg[k] = rint(log2(k) Q) for k = 1 .. tau_max, built by the caller in float64 (entry 0 is not read); the
 *             library computes no logarithm
 *   costs   : unvoiced_q, octave_q, jump_q, vuv_q: int32, rint((double) value * Q), each in 0 .. 16 Q
 *   q(x)    = x < 4.0f ? (int) rintf(x * 65536.f) : 4 Q, so NaN and +inf land on 4 Q.  d' is never negative; an x at or below -4 -- outside
 *             what efts_yin writes -- counts as -4 Q.
 *   obs(t, s) = q(cmnd[t][k]) + (((int64) octave_q * (lg[k] - lg[tau_min])) >> 16) for a voiced state;  obs(t, S) = unvoiced_q
 *   trans   : voiced k' -> voiced k: ((int64) jump_q * |lg[k] - lg[k']|) >> 16;  voiced <-> unvoiced: vuv_q;  unvoiced -> unvoiced: 0
 * Recurrence:
 *   C(0, s) = obs(0, s);   C(t, s) = obs(t, s) + min over p of (C(t - 1, p) + trans(p, s))
 *   ties: the predecessor with the lowest state index wins; the final state is the lowest index among the minima of C(n - 1, .); the path
 *   is traced back from there.  The path is exact for every T the call admits: each frame is stored less the minimum of the frame before,
 *   which moves no argmin, so 32 bits never overflow.
 * Outputs, [B][T] each, for t < n with k the lag of the path's state at t:
 *   lag          : int32, k, or 0 for the unvoiced state
 *   f0           : voiced: sampling_rate / (k + shift) with efts_yin's parabola AT k (no walk to a local minimum): fp32, s0, s1, s2 =
 *                  d'(k - 1), d'(k), d'(k + 1), den = (s0 - s1) + (s2 - s1), shift = 0.5 (s0 - s2) / den clamped to [-1, 1], 0 when den == 0.
 *                  Unvoiced: 0.
 *   aperiodicity : voiced: d'(k).  Unvoiced: the smallest d' over the lags tau_min .. tau_max - 1 (fminf: a NaN is passed over).
 *   All three are 0 for n <= t < T.
 * workspace : device memory, 16-byte aligned, B times what the workspace-size entry returns for the same (T, tau_min, tau_max): one uint16
 *   back-pointer per (frame, state), T (S + 1) 2 bytes per item rounded up to 16.  workspace_bytes is what the caller holds.  Contents
 *   afterwards: unspecified.  The size entry returns 0 for arguments that the call would refuse; it is monotone in T and in S.
 * One launch, one workgroup per item, no atomics: an item gives the same bits alone, in any batch position and in any run.
 * EFTS_EINVAL: null pointer.  EFTS_ESHAPE, nothing launched: a lag range outside the above, B outside 1 .. 65535, T outside
 * 1 .. EFTS_VITERBI_MAX_FRAMES, sampling_rate < 1, frame_stride < tau_max + 1, item_stride < 0, a cost outside 0 .. 16 Q, a workspace smaller
 * than B items need.  EFTS_EALIGN: workspace misaligned.
 * ---------------------------------------------------------------------------------- */
#define EFTS_VITERBI_MAX_LAG 1024
#define EFTS_VITERBI_MAX_FRAMES 1048576
int64_t efts_f0_viterbi_workspace_bytes(int32_t T, int32_t tau_min, int32_t tau_max);
int efts_f0_viterbi(const float* cmnd, int64_t item_stride, int64_t frame_stride, const int32_t* frames, const int32_t* lg, float* f0,
                    float* aperiodicity, int32_t* lag, void* workspace, int64_t workspace_bytes, int32_t B, int32_t T, int32_t tau_min,
                    int32_t tau_max, int32_t sampling_rate, int32_t unvoiced_q, int32_t octave_q, int32_t jump_q, int32_t vuv_q, void* stream);

/* ------------------------------------------------------------------------------------
 * Silence trimming and peak normalisation of a padded batch: the quiet ends of every item are cut off and what is left is scaled.
 * Parameters: frame length W (512, 1024 or 2048), hop H (1 <= H <= W, W - H even), pad = (W - H) / 2, the threshold ratio
 * r = 10^(top_db / 10) > 1 (computed by the caller in double), keep_frames, peak (<= 0: no normalisation), and on the int16 entry pcm_scale
 * (1 / max_wav_value).  For item b with len = lengths[b] (clamped to 0 .. ld_in) samples x, x = 0 outside [0, len):
 *   frames    : T = ceil(len / H); frame t covers samples t H - pad .. t H - pad + W - 1; its energy E_t is the sum of x^2 over the frame.
 *               int16: the exact integer sum of the raw sample values in an unsigned 64-bit accumulator (at most 2048 * 2^30 = 2^41: every
 *               order gives the same value).
 *               fp32, ONE fixed order: a frame is R segments of S samples, segment j of the item starting at sample j H - pad; S = H and
 *               R = W / H when H divides W and H >= 64, else S = W and R = 1.  Segment sum P_j: lane l = 0 .. 63 starts from 0 and takes
 *               acc = fma(x_i, x_i, acc) over the segment's samples i = l, l + 64, l + 128, ... in ascending order; the 64 lane sums are
 *               then combined by v = v + (the v of the lane 32 across), then 16, 8, 4, 2, 1 across (every lane ends with the same bits).
 *               E_t = (..((P_t + P_{t+1}) + P_{t+2}) ..) + P_{t+R-1}.  Samples are addressed by their index in the item, never by their
 *               address, so the order does not depend on where the row lies.
 *   threshold : E_max = max over t of E_t.  Frame t is SOUND iff (double) E_t * r > (double) E_max: one correctly rounded fp64 multiply and
 *               one compare.  E_max == 0 (an empty or all-zero item): no frame is sound.
 *   bounds    : t_first / t_last the first / last sound frame: start = max(0, (t_first - keep_frames) H),
 *               end = min(len, (t_last + 1 + keep_frames) H).  No sound frame: start = 0, end = len and the gain is 1.  new_len = end - start.
 *               keep_frames < 0 switches the trimming off: every item keeps 0 .. len (normalisation alone).
 *   gain      : p = max |x_i| over start <= i < end (exact; int16: of the raw integers).  With peak > 0 and p > 0: g = (float) peak / (float) p,
 *               one correctly rounded fp32 division.  Otherwise g = pcm_scale on the int16 entry and 1 on the fp32 entry.
 *   out[b * ld_out + i] = (float) x[start + i] * g for i < new_len, exactly 0.0f for new_len <= i < ld_out.
 *   new_len, start (int32 [B]) and gain (fp32 [B]) are written by the kernels.
 * No sample at or beyond len and no other row is read or influences anything; an item gives the same bits alone, at any batch position and
 * in any run (no atomics).  lengths[b] == 0 is legal: zeros, new_len 0, gain 1.
 * workspace : device memory, 16-byte aligned, of the size that the workspace-size entry returns for (B, max_len = ld_in, H, pcm16 = 0 for
 *             the fp32 entry and 1 for the int16 entry): the frame energies [B][T_max] (uint64 or fp32) and, behind them, the peak of every
 *             hop chunk c H .. c H + H - 1 [B][T_max] (int32 or fp32), T_max = ceil(ld_in / H).  Contents afterwards: unspecified.  The
 *             size entry returns 0 for a non-positive argument.
 * Three launches: energies and chunk peaks (the samples are read once, 16 bytes at a time where the row's address allows), the per-item
 * decision on the workspace alone, and the compacting, scaling copy.  No host synchronisation, no allocation.
 * EFTS_ESHAPE, nothing launched: B outside 1 .. 65535, ld_in < 1, ld_out < ld_in, either near 2^31, W other than 512, 1024, 2048, H outside
 * 1 .. W or W - H odd.  EFTS_EINVAL: null pointer, a pointer not aligned to its element (the workspace: to 16 bytes), r <= 1.
 * ---------------------------------------------------------------------------------- */
int64_t efts_trim_workspace_bytes(int32_t B, int64_t max_len, int32_t H, int32_t pcm16);
int efts_trim(const float* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t keep_frames, float peak, float* out,
              int64_t ld_out, int32_t* new_len, int32_t* start, float* gain, void* workspace, int32_t B, void* stream);
int efts_trim_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t keep_frames, float peak,
                    float pcm_scale, float* out, int64_t ld_out, int32_t* new_len, int32_t* start, float* gain, void* workspace, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * Shortening the long pauses INSIDE the items of a padded batch: every run of quiet hop chunks between two sound frames that is longer than
 * M chunks is cut down to M chunks, and what is kept is moved together, with a linear fade into the joint.
 * Parameters: W, H, pad = (W - H) / 2 and r = 10^(top_db / 10) > 1 as for efts_trim; M >= 1, the longest pause in chunks that is kept whole
 * (the caller computes M = max(1, round(max_pause_ms * sampling_rate / (1000 H))) and passes it by value); the fade length 0 <= F <= H and
 * the fade table w[0 .. F), w_k = (k + 0.5) / F computed in double and rounded once to fp32 by the caller; on the int16 entry pcm_scale
 * (1 / max_wav_value).  For item b with len = lengths[b] (clamped to 0 .. ld_in) samples x, x = 0 outside [0, len):
 *   frames    : T, the frame energies E_t, E_max and the SOUND rule, (double) E_t * r > (double) E_max, are those of efts_trim above, word for
 *               word: int16 energies are exact 64-bit integers, fp32 energies are summed in the one order stated there.
 *   chunks    : chunk c is samples c H .. c H + H - 1 (the last one ends at len); it is QUIET iff frame c is not sound.  t_first / t_last are
 *               the first / last sound frame.  No sound frame: the item comes back as it is (int16: scaled), removed = 0, pauses = 0.
 *   pauses    : a PAUSE is a maximal run of quiet chunks [c0, c1) with t_first < c0 and c1 <= t_last.  The quiet chunks in front of t_first
 *               and behind t_last are no pauses and stay where they are (efts_trim cuts those).  Every pause lies between two sound
 *               chunks, so every chunk of it is a whole chunk.
 *   plan      : a pause of n = c1 - c0 <= M chunks is kept whole.  A pause of n > M chunks keeps its first head = (M + 1) / 2 and its last
 *               tail = M / 2 chunks (integer division) and loses the n - M chunks between them: with a = (c0 + head) H and
 *               b = (c1 - tail) H, samples [a, b) are removed.  removed = the sum of (n - M) H over these pauses (a multiple of H),
 *               pauses = their number, new_len = len - removed.
 *   chunk_src : the kept chunks in ascending order: chunk_src[j] is the source chunk of output chunk j, for j < T - removed / H, and -1 for
 *               every j behind, up to T_max = ceil(ld_in / H).  It maps positions in the shortened signal back onto the recording.
 *   samples   : out[j H + k] = (float) x[chunk_src[j] H + k] for j H + k < new_len: the bits of the sample (int16: one correctly rounded
 *               fp32 multiply, (float) sample * pcm_scale), except on the last F samples in front of a joint: there, for k = 0 .. F - 1,
 *               the output sample at the position of x[a - F + k] is fmaf(w_k, x[b - F + k] - x[a - F + k], x[a - F + k]) -- one correctly
 *               rounded fp32 subtraction and one fused multiply-add, every x the fp32 value (int16: (float) sample * pcm_scale).  Both
 *               operand ranges lie inside the pause (F <= H and head >= 1 on the left, one removed chunk on the right), and the output runs
 *               continuously into x[b].  F = 0 is a plain cut.  Exactly 0.0f for new_len <= i < ld_out.
 *   new_len, removed, pauses (int32 [B]) and chunk_src (int32 [B][T_max]) are written by the kernels.
 * No sample at or beyond len and no other row is read or influences anything; an item gives the same bits alone, at any batch position and
 * in any run (no atomics).  lengths[b] == 0 is legal: zeros, new_len 0.
 * workspace : device memory, 16-byte aligned, of the size that the workspace-size entry returns for (B, max_len = ld_in, H, pcm16 = 0 for
 *             the fp32 entry and 1 for the int16 entry): the frame energies [B][T_max] (uint64 or fp32) and two int32 [B][T_max] arrays of the
 *             plan.  Contents afterwards: unspecified.  The size entry returns 0 for a non-positive argument.
 * Three launches on the caller's stream: the energies (efts_trim's launch without the chunk peaks), the plan (one workgroup per item, which
 * walks the T chunks in tiles of EFTS_PAUSES_TILE and carries its scans from tile to tile: an item of any length below 2^31 samples), and the
 * compacting copy over (item, output chunk), 16 bytes per access where both rows are 16-byte aligned and the hop is a multiple of the
 * samples in 16 bytes.  No host synchronisation, no allocation, no launch geometry from device data.
 * EFTS_ESHAPE, nothing launched: B outside 1 .. 65535, ld_in < 1, ld_out < ld_in, either near 2^31, W other than 512, 1024, 2048, H outside
 * 1 .. W or W - H odd, M outside 1 .. 2^30, F outside 0 .. H.  EFTS_EINVAL: null pointer (the fade table only with F > 0), a pointer not
 * aligned to its element (the workspace: to 16 bytes), r <= 1.
 * ---------------------------------------------------------------------------------- */
#define EFTS_PAUSES_TILE 256
int64_t efts_pauses_workspace_bytes(int32_t B, int64_t max_len, int32_t H, int32_t pcm16);
int efts_pauses(const float* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t M, int32_t F, const float* fade,
                float* out, int64_t ld_out, int32_t* new_len, int32_t* removed, int32_t* pauses, int32_t* chunk_src, void* workspace, int32_t B,
                void* stream);
int efts_pauses_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t M, int32_t F,
                      const float* fade, float pcm_scale, float* out, int64_t ld_out, int32_t* new_len, int32_t* removed, int32_t* pauses,
                      int32_t* chunk_src, void* workspace, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * STFT magnitudes and the STFT distance between two signals at one resolution (N, H, W): FFT size N (256, 512, 1024 or 2048), hop
 * 1 <= H <= N, window length 2 <= W <= N.  Replaces nntts/losses/stft_loss.py: stft (:12-32), SpectralConvergenceLoss (:53),
 * LogSTFTMagnitudeLoss (:74); MultiResolutionSTFTLoss (:110) is one call per resolution.
 *   samples : fp32, or int16 PCM (pcm16 != 0) multiplied by pcm_scale (1 / max_wav_value) at the load; an fp32 signal is not scaled.
 *             Item b is row b of its [B][ld] array and has len = lengths[b], clamped to 0 .. max_len, samples; nothing behind them is read.
 *   window  : [W] fp32, DEVICE memory: the periodic Hann window w[i] = 0.5 - 0.5 cos(2 pi i / W), computed by the caller in float64 and
 *             rounded once.  It sits in the N-sample frame with (N - W) / 2 (integer division) zeros in front, as torch.stft places it.
 *   frames  : an item has T = 1 + len / H frames when len > N / 2, and none otherwise (it cannot be reflect-padded).  Sample n of frame t is
 *             index i = t H - N / 2 + n of the signal, reflected without edge repeat: i < 0 -> -i, i >= len -> 2 (len - 1) - i.
 *   spectrum: the fp32 N-point DFT of the windowed frame; mag[t][f] = sqrt(max(re^2 + im^2, 1e-7)) for f = 0 .. N / 2.  Frames 2 p and
 *             2 p + 1 of a signal share one complex transform; both signals of efts_stft_dist pass through the same instructions, so equal
 *             samples give equal magnitudes.
 * efts_stft_mag: mag [B][T_max][N / 2 + 1], T_max = 1 + max_len / H; rows at and beyond an item's T are 0.  frames [B] int32: T.
 * efts_stft_dist: x is the candidate, y the reference signal.  Per item, over its own T (N / 2 + 1) cells:
 *   sums [B][3] float64: num = sum (mag_y - mag_x)^2, den = sum mag_y^2, l1 = sum |ln mag_y - ln mag_x|;  cells [B] int64: T (N / 2 + 1).
 *   An item without frames has cells = 0 and sums 0: the device decides, nothing is read back.  From these,
 *   spectral convergence = sqrt(num) / sqrt(den) and log-magnitude distance = l1 / cells.
 *   ONE fixed order.  Inside a frame, fp32: with G = 16, 32, 64, 64 lanes for N = 256, 512, 1024, 2048, lane l starts from 0 and takes its
 *   bins f = l, l + G, l + 2 G, ... in ascending order -- num = fma(d, d, num) with d = mag_y - mag_x, den = fma(mag_y, mag_y, den),
 *   l1 = l1 + |ln mag_y - ln mag_x| -- and the G lane sums are combined by v = v + (the v of the lane G / 2 across), then G / 4, .., 1
 *   across.  Across an item's frames: float64, frame 0 first, one addition per frame, by a second launch.  No atomics: an item gives the
 *   same bits alone, at any batch position, in any run and whatever lies behind its samples.
 *   workspace: device memory, 16-byte aligned, of the size the workspace-size entry returns (three fp32 per frame: [B][T_max][3]);
 *   contents afterwards unspecified.  The size entry returns 0 for arguments the call would refuse.
 * EFTS_EINVAL, nothing launched, the entry's name in efts_last_error(): N other than the four sizes, H or W out of range, B outside
 * 1 .. 65535, max_len outside 1 .. 2^31 - 8193, a leading dimension below max_len, a workspace too small, a null or misaligned pointer.
 * ---------------------------------------------------------------------------------- */
int efts_stft_mag(const void* audio, int32_t pcm16, float pcm_scale, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window,
                  float* mag, int32_t* frames, int32_t B, int32_t N, int32_t H, int32_t W, void* stream);
int64_t efts_stft_dist_workspace_bytes(int32_t B, int32_t max_len, int32_t N, int32_t H);
int efts_stft_dist(const void* x, int32_t x_pcm16, int64_t ldx, const void* y, int32_t y_pcm16, int64_t ldy, float pcm_scale, const int32_t* lengths,
                   int32_t max_len, const float* window, double* sums, int64_t* cells, void* workspace, int64_t workspace_bytes, int32_t B, int32_t N,
                   int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------------------------
 * Integrated loudness after ITU-R BS.1770 / EBU R 128 of a padded batch, and the gain that brings every item to a target loudness.
 * Parameters: the sampling rate fs (8000 .. 48000 Hz, a multiple of 10), kweight (HOST memory, ten doubles, read during the call: the
 * K-weighting coefficients that the caller computed once in float64 -- shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2, a0 = 1 in both),
 * target_lufs, peak_ceiling (<= 0: no ceiling) and on the int16 entry pcm_scale (1 / max_wav_value).  For item b with len = lengths[b]
 * (clamped to 0 .. ld_in) samples x_i = (double) in[i] (int16: (double) in[i] * (double) pcm_scale), x = 0 outside [0, len):
 *   K-weighting: y = HP(SHELF(x)), two biquads in transposed direct form II, fp64, per sample and in this order of operations:
 *               v = fma(sb0, x, s1); s1 = fma(-sa1, v, fma(sb1, x, s2)); s2 = fma(-sa2, v, sb2 * x);
 *               y = fma(hb0, v, t1); t1 = fma(-ha1, y, fma(hb1, v, t2)); t2 = fma(-ha2, y, hb2 * v).
 *               The coefficients are the bilinear designs of libebur128, which give the standard's table at 48 kHz.  Shelf: f0 =
 *               1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *               Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2, b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0,
 *               (Vh - Vb K / Q + K^2) / a0], a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0.  High-pass: f0 = 38.13547087602444,
 *               Q = 0.5003270373238773, K = tan(pi f0 / fs), b = [1, -2, 1], a1 = 2 (K^2 - 1) / (1 + K / Q + K^2),
 *               a2 = (1 - K / Q + K^2) / (1 + K / Q + K^2).
 *   the recurrence in parallel: the item is cut into segments of EFTS_LOUDNESS_SEGMENT samples, segment s = samples s SEG .. s SEG + SEG - 1.
 *               Every segment is filtered on its own: from ZERO state at sample max(0, s SEG - 2 h), h = fs / 10, so that 0.2 s of warm-up lie
 *               in front of its first sample.  Segments that start within the first 2 h samples are exact (x = 0 in front of the item is the
 *               zero state); for the others, what the 38 Hz high-pass (the slowest pole: radius 0.995 at 48 kHz) still holds of input more
 *               than 0.2 s back is dropped.  Against a strictly sequential float64 filter that is a relative error of y below 2e-13 (measured
 *               at 48 kHz with a warm-up of 8192 samples = 0.171 s on gated noise with a DC offset; the decay is a matter of time, so 2 h
 *               samples do at least as well at every rate); 4096 samples at 48 kHz would give 2e-9, 2048 2.9e-5.
 *   sub-blocks: h samples each; sub-block k = samples k h .. k h + h - 1, nb = floor(len / h) of them.  Every segment adds y^2 of its samples,
 *               in ascending order with acc = fma(y, y, acc) from 0, into one part per sub-block that it touches (at most two, SEG <= h);
 *               U_k = the parts of sub-block k added in ascending order of their segments, from 0.
 *   blocks    : block j = 0 .. nb - 4 is sub-blocks j .. j + 3 (400 ms at a hop of 100 ms): z_j = (((U_j + U_j+1) + U_j+2) + U_j+3) * (1 / (4 h)).
 *               Fewer than four whole sub-blocks: no block.
 *   gate      : in the z domain, no logarithm decides anything.  Ga = 10^((-70 + 0.691) / 10); A = { j : z_j > Ga }; Gr = 0.1 * mean(z_j, j in A);
 *               G = { j in A : z_j > Gr };  L = -0.691 + 10 log10(mean(z_j, j in G)).  A mean is sum / count, its sum in ONE order: thread
 *               t = 0 .. 255 adds its members among j = t, t + 256, t + 512, ... in ascending order from 0; inside each of the four waves
 *               v = v + (the v of the lane 32 across), then 16, 8, 4, 2, 1 across; then ((wave 0 + wave 1) + wave 2) + wave 3.
 *               No block at all, or an empty A: L = -inf and flag bit 0 is set.
 *   gain      : g = 10^((target_lufs - L) / 20), p = max |x_i| over the item.  With peak_ceiling > 0 and g p > peak_ceiling: flag bit 1 is set
 *               and the gain becomes the largest fp32 not above peak_ceiling / p (times pcm_scale on the int16 entry) for which
 *               (float) max |in[i]| * gain, rounded to fp32, is not above peak_ceiling: no output sample exceeds the ceiling.  Otherwise
 *               gain = (float) g (int16: (float) (g * pcm_scale)), rounded to nearest once.  L = -inf: g = 1, no ceiling applies.
 *   out[b * ld_out + i] = (float) in[i] * gain for i < len, exactly 0.0f for len <= i < ld_out.  out == NULL: measurement only, ld_out is
 *   ignored and the copy is not launched.
 *   loudness (double [B]: L), gain (fp32 [B]), flags (int32 [B]) and blocks (int32 [B][2]: |A| and |G|) are written by the kernels.
 * No sample at or beyond len and no other row is read or influences anything; no atomics: an item gives the same bits alone, at any batch
 * position and in any run.  lengths[b] == 0 is legal.
 * workspace : device memory, 16-byte aligned, of the size that the workspace-size entry returns for (B, max_len = ld_in, fs): the parts
 *             [B][ceil(ld_in / SEG)][2] fp64, the segment peaks [B][ceil(ld_in / SEG)] fp32 and the sub-block sums [B][ld_in / h + 1] fp64.
 *             Contents afterwards: unspecified.  The size entry returns 0 for arguments the call would refuse.
 * Three launches (two without out): the filter with the parts and segment peaks (one thread per segment; bound by the latency of the fp64
 * recurrence, not by bytes), the per-item decision on the workspace alone, and the scaling copy.  No host synchronisation, no allocation.
 * EFTS_ESHAPE, nothing launched: B outside 1 .. 65535, ld_in < 1, ld_out < ld_in (with out), either near 2^31, fs outside 8000 .. 48000 or
 * not a multiple of 10.  EFTS_EINVAL: a null pointer other than out, a pointer not aligned to its element (the workspace: to 16 bytes), a
 * target or coefficient that is not finite, a NaN ceiling, pcm_scale not a positive number.
 * ---------------------------------------------------------------------------------- */
#define EFTS_LOUDNESS_SEGMENT 512
int64_t efts_loudness_workspace_bytes(int32_t B, int64_t max_len, int32_t fs);
int efts_loudness(const float* in, int64_t ld_in, const int32_t* lengths, int32_t fs, const double* kweight, double target_lufs, double peak_ceiling,
                  float* out, int64_t ld_out, double* loudness, float* gain, int32_t* flags, int32_t* blocks, void* workspace, int32_t B, void* stream);
int efts_loudness_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, int32_t fs, const double* kweight, double target_lufs,
                        double peak_ceiling, float pcm_scale, float* out, int64_t ld_out, double* loudness, float* gain, int32_t* flags,
                        int32_t* blocks, void* workspace, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * Spectral denoiser for a vocoder's bias noise: STFT -> subtract strength * bias from the magnitudes, clamp at 0, keep the phase -> inverse
 * STFT -> overlap-add, in one launch.  What the published Tacotron 2 / WaveGlow / HiFi-GAN inference scripts do with torch.stft / torch.istft.
 * Fixed configuration: N = 1024, H = 256, W = 1024, everything fp32; the entry takes no argument that could ask for another one (a later
 * entry that does refuses what it was not built for with EFTS_ESHAPE).
 *   samples : fp32.  Item b is row b of audio [B][ld] and has len = lengths[b], clamped to 0 .. max_len, samples; nothing behind them is read.
 *   window  : [1024] fp32, DEVICE memory: the periodic Hann window w[i] = 0.5 - 0.5 cos(2 pi i / 1024), computed by the caller in float64 and
 *             rounded once; the same window for analysis and synthesis.
 *   bias    : [513] fp32, DEVICE memory: non-negative magnitudes per bin.  strength: a finite float >= 0, passed by value.
 *   frames  : exactly those of efts_stft_mag: an item has T = 1 + len / 256 frames when len > 512.  Sample n of frame t is index
 *             i = 256 t - 512 + n of the signal, reflected without edge repeat: i < 0 -> -i, i >= len -> 2 (len - 1) - i.
 *   per frame: X = DFT(w * frame) for f = 0 .. 512; m = sqrt(fma(re, re, im * im)); d = m - strength * bias[f]; g = d / m if d > 0, otherwise
 *             0 (so g = 0 where m = 0); X' = g X; x' = the real inverse DFT of X' (the imaginary parts of DC and Nyquist are dropped).
 *   out[b * ld_out + s] = (sum over the frames t that cover s, oldest first, of w[n] * x'_t[n], n = s + 512 - 256 t) / max(sum of their w[n]^2, 1e-8)
 *             for s < len, exactly 0.0f for len <= s < ld_out.  This is torch.stft(center=True, pad_mode="reflect") -> gain ->
 *             torch.istft(center=True, length=len).
 *   An item with len <= 512 cannot be reflect-padded: its samples are copied to out bit for bit and frames[b] = 0.  frames [B] int32: T.  The
 *   device decides; nothing is read back.
 *   ONE fixed order, no atomics.  Frames 2 p and 2 p + 1 of an item share one complex transform, forward and inverse (frame 2 p the real
 *   part; an unpaired last frame has a zero partner whose gain is 0); a pair never crosses items.  A run of 16 consecutive hops (hop c =
 *   samples 256 c .. 256 c + 255; runs begin at multiples of 16 hops of the item) is overlap-added by one wave, which computes frames
 *   c0 - 2 .. c0 + 17 of its run c0 .. c0 + 15 itself: every sample starts from 0 and receives w[n] * x'_t[n] of its up to four frames in
 *   ascending t, the sum of w[n]^2 likewise, then one division.  An item gives the same bits alone, at any batch position, in any run and
 *   whatever lies behind its samples.  No spectrum and no frame goes to memory.
 *   workspace: none is needed: the size entry returns 0 for every argument, workspace may be NULL (or 16-byte aligned) and is not touched.
 * EFTS_EINVAL, nothing launched, the entry's name in efts_last_error(): a null pointer (other than workspace) or one not aligned to its
 * element, B outside 1 .. 65535, max_len outside 1 .. 2^31 - 8193, a leading dimension below max_len, ld_out >= 2^31, a negative or
 * non-finite strength, workspace_bytes < 0, out [B][ld_out] overlapping audio.
 * ---------------------------------------------------------------------------------- */
int64_t efts_denoise_workspace_bytes(int32_t B, int32_t max_len);
int efts_denoise(const float* audio, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window, const float* bias, float strength,
                 float* out, int64_t ld_out, int32_t* frames, void* workspace, int64_t workspace_bytes, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * Short-time objective intelligibility: STOI (Taal, Hendriks, Heusdens, Jensen 2011) and ESTOI (Jensen, Taal 2016) of a processed signal y
 * against the clean signal x, time-aligned and both at 10 000 Hz, as the authors' Matlab code computes them (which pystoi follows), quirks
 * included.  Fixed configuration: frame 256, hop 128, FFT 512 (the frame followed by 256 zeros), J = 15 one-third-octave bands from 150 Hz,
 * segments of N = 30 frames, beta = -15 dB, dynamic range 40 dB; the entry takes no argument that could ask for another one.
 *   samples : fp32.  Item b is row b of x [B][ldx] and of y [B][ldy] and is compared over n = lengths[b], clamped to 0 .. max_len, samples;
 *             nothing behind them is read.
 *   window  : [256] fp32, DEVICE memory: w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257) (numpy's hanning(258)[1:-1]), computed by the caller in
 *             float64 and rounded once.
 *   1 frames   : F = (n - 256) / 128 + 1 when n >= 256, otherwise 0.  Frame f of a signal s is w[i] s[128 f + i], i = 0 .. 255.
 *   2 silent frames, decided on x alone: e[f] = sum_i (w[i] x[128 f + i])^2 in fp32 -- lane l of a wave takes i = l + 64 j, j = 0 .. 3: s = 0,
 *             v = w[i] x[..] (rounded), s = fmaf(v, v, s) in ascending j; then s += (s of lane l xor 32), xor 16, 8, 4, 2, 1.  e_max = max_f
 *             e[f].  Frame f is kept iff (double) e[f] * 10^4 > (double) e_max, strictly: the reference's 20 log10 ||frame|| > max - 40
 *             without a logarithm deciding anything, and without the eps inside the reference's logarithm, so an all-zero x keeps
 *             nothing.  k_0 < k_1 < .. < k_(K-1) are the kept frames; the same frames are kept from y.
 *   3 compacted signals: the kept windowed frames overlap-added at hop 128: xs[p] = sum over the at most two j that cover p, in ascending
 *             j, of w[p - 128 j] x[128 k_j + p - 128 j] -- the older product rounded, the younger one fused onto it (fmaf) --; ys likewise.
 *             They have 128 (K - 1) + 256 samples and never exist in memory.
 *   4 spectral frames: T = K - 1 (the reference's loop stops before the last frame).  Frame t holds w[i] xs[128 t + i]; it needs the kept
 *             frames k_(t-1) (second half; absent at t = 0), k_t and k_(t+1) (first half).  The x frame and the y frame run as ONE complex
 *             512-point fp32 transform z = x frame + i y frame; X[f] = (Z[f] + conj Z[512 - f]) / 2, Y[f] = (Z[f] - conj Z[512 - f]) / 2i;
 *             P[t][f] = fmaf(re, re, im im).
 *   5 bands    : X[t][j] = sqrt(sum_{f = lo_j}^{hi_j - 1} P[t][f]), fp32, in ascending f, with [lo, hi) = [7,9) [9,11) [11,14) [14,17) [17,22)
 *             [22,27) [27,34) [34,43) [43,55) [55,69) [69,87) [87,109) [109,138) [138,174) [174,219): the bins nearest to
 *             150 2^((2 j -+ 1) / 6) Hz on the grid f 10000 / 512, upper bin excluded.  Y[t][j] likewise from y's spectrum.
 *   6 segments : M = T - 29 = K - 30 when K > 30, otherwise there is none.  Segment m is the [15][30] block X[m .. m + 29][.] transposed, Y
 *             likewise; from here on everything is float64, eps = 2^-52.  A sum over the 30 frames of a segment is the xor tree over 32
 *             lanes (lane n holds frame n, lanes 30 and 31 hold 0: v += v of lane n xor 16, then 8, 4, 2, 1); a sum over the 15 bands
 *             runs in ascending j.
 *             STOI, per band j: c = ||x_j|| / (||y_j|| + eps); y' = min(c y_j, x_j (1 + 10^(15/20))); x_j and y' minus their means (sum / 30),
 *             each divided by (its norm + eps); d_mj = sum over the frames of their product.  stoi = (sum_m (sum_j d_mj)) / (15 M).
 *             ESTOI: both blocks are normalised alike: every row (a band over the 30 frames) minus its mean, divided by (its norm + eps);
 *             then every column (a frame over the 15 bands) minus its mean (sum / 15), divided by (its norm + eps) (squares and products
 *             summed with fma).  estoi = (sum_m (sum over the frames of (sum_j x~ y~))) / (30 M).
 *             The segments' sums are added per item in ascending m.
 *   stoi, estoi [B] float64; frames, kept, segments [B] int32: F, K and M.  An item without a segment (F = 0, K <= 30, an all-zero x) gets
 *   NaN in both scores and segments = 0: the reference code warns and returns 1e-5 there.  The device decides; nothing is read back, no
 *   launch geometry depends on device data, and the call can be captured.  ONE fixed order, no atomics: an item gives the same bits
 *   alone, at any batch position and whatever lies behind its samples.
 *   workspace: efts_stoi_workspace_bytes(B, max_len) bytes, 16-byte aligned; the size entry returns 0 for arguments that efts_stoi refuses.
 * EFTS_EINVAL, nothing launched, the entry's name in efts_last_error(): a null pointer or one not aligned to its element, B outside
 * 1 .. 65535, max_len outside 1 .. 2^31 - 8193, a leading dimension below max_len, a workspace smaller than the size entry asks for.
 * ---------------------------------------------------------------------------------- */
int64_t efts_stoi_workspace_bytes(int32_t B, int32_t max_len);
int efts_stoi(const float* x, int64_t ldx, const float* y, int64_t ldy, const int32_t* lengths, int32_t max_len, const float* window, double* stoi,
              double* estoi, int32_t* frames, int32_t* kept, int32_t* segments, void* workspace, int64_t workspace_bytes, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * A linear map of the log power spectrum of every frame of a waveform batch, in one launch, and the summed distance between the frames of
 * two feature sequences paired one to one.  With the table of efficient_tts_amd/mcep.py the first gives mel-cepstra of waveforms -- the
 * all-pass frequency transform (Oppenheim's recursion, SPTK's freqt) of the FFT cepstrum of the periodogram, without the level c0 -- and
 * both give the mel-cepstral distortion that TTS and vocoder papers report.  The entries themselves know nothing about cepstra.
 * efts_logspec_project:
 *   framing : that of efts_stft_mag, exactly, at N = 1024 only: hop 1 <= H <= N, the periodic Hann window [W] (2 <= W <= N, DEVICE memory)
 *             with (N - W) / 2 zeros in front, reflect padding without edge repeat, T = 1 + len / H frames when len > N / 2 and none
 *             otherwise, len = lengths[b] clamped to 0 .. max_len, int16 PCM (pcm16 != 0) multiplied by pcm_scale at the load, frames 2 p
 *             and 2 p + 1 through one complex transform.  Nothing behind an item's samples is read.
 *   power   : P[t][f] = max(re^2 + im^2, 1e-7) for f = 0 .. K, K = N / 2 -- the clamp of efts_stft_mag, applied before its square root, the
 *             same bits -- and L[t][f] = ln P[t][f] (fp32 logf).
 *   project : out[b][t][k] = sum_f table[k][f] L[t][f], k < n_coef; table [n_coef][K + 1] fp32 in DEVICE memory, 1 <= n_coef <= 32.
 *             fp32, ONE fixed order: lane l of 64 starts from 0 and takes its bins f = l, l + 64, .., (lane 0: .., 512) in ascending order,
 *             s = fma(table[k][f], L[f], s); the 64 lane sums are combined by v = v + (the v of the lane 32 across), then 16, .., 1 across.
 *   out [B][T_max][n_coef], T_max = 1 + max_len / H; rows at and beyond an item's T are 0.  frames [B] int32: T.
 *   No spectrum goes to memory, no atomics, no launch geometry from device data; the call can be captured.  An item gives the same bits
 *   alone, at any batch position, in any run and whatever lies behind its samples.
 *   The table of mel-cepstra (built by the caller in float64, rounded once to fp32): rows 1 .. M of  1/2 A(alpha) diag(w) D,  where
 *   D[n][f] = s_f cos(pi n f / K) / K with s_0 = s_K = 1 and s_f = 2 otherwise, w_0 = w_K = 1/2 and w_n = 1 otherwise -- so that
 *   c = diag(w) D ln|X| is the one-sided cepstrum, ln|X(w_f)| = sum_{n = 0 .. K} c[n] cos(n w_f) exactly, and the factor 1/2 turns ln P
 *   into ln|X| --, and A(alpha) is the (M + 1) x (K + 1) matrix of the recursion: g = 0, beta = 1 - alpha^2; for i = K down to 0, with d the
 *   previous g:  g[0] = c[i] + alpha d[0],  g[1] = beta d[0] + alpha d[1],  g[j] = d[j - 1] + alpha (d[j] - g[j - 1]) for j = 2 .. M.
 *   Row 0, the level, is left out, as efts_mel_cepstrum leaves it out.
 * efts_frame_dist: x [B] items of rows of D <= 32 fp32 (row stride ldx, item stride x_item_stride, in elements), x_frames [B] int32 clamped
 *   to 0 .. Tx; y likewise.  n = min of the two clamped frame counts;  cost[b] (float64) = sum over t = 0 .. n - 1, in ascending t, one
 *   float64 addition per frame, of d(t, t), the local cost of efts_dtw: sqrt (correctly rounded, fp32) of s = fma(x[t][k] - y[t][k], the same,
 *   s) over ascending k.  count[b] = n.  An item without frames gets NaN and 0.  One workgroup per item, no atomics; rows at and beyond n
 *   are never read.
 * From either, mcd = (10 / ln 10) sqrt(2) cost / count dB, cost and count those of efts_dtw (warped) or of efts_frame_dist (aligned).
 * Nothing launched and the entry's name in efts_last_error(): EFTS_ESHAPE for N other than 1024, H, W, n_coef, D or B (1 .. 65535) out of
 * range, max_len outside 1 .. 2^31 - 8193, a leading dimension below max_len, a row stride below D, a negative item stride, Tx or Ty below 1;
 * EFTS_EINVAL for a null pointer or one not aligned to its element.
 * ---------------------------------------------------------------------------------- */
int efts_logspec_project(const void* audio, int32_t pcm16, float pcm_scale, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window,
                         const float* table, int32_t n_coef, float* out, int32_t* frames, int32_t B, int32_t N, int32_t H, int32_t W, void* stream);
int efts_frame_dist(const float* x, int64_t ldx, int64_t x_item_stride, const int32_t* x_frames, int32_t Tx, const float* y, int64_t ldy,
                    int64_t y_item_stride, const int32_t* y_frames, int32_t Ty, int32_t D, double* cost, int32_t* count, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * Spectral gating of a corpus with a noise profile per recording: the stationary floor under the speech (room tone, fan noise, hiss) is
 * measured from every item's own quiet frames and subtracted from its magnitudes, with a floor under the gain.  Fixed configuration, that of
 * efts_denoise: N = 1024, H = 256, W = 1024; samples fp32, or int16 PCM (pcm16 != 0) multiplied by pcm_scale (1 / max_wav_value) at the load,
 * x = fl32((float) sample * pcm_scale); an fp32 signal is not scaled.  Item b is row b of audio [B][ld] and has len = lengths[b], clamped to
 * 0 .. max_len, samples; nothing behind them is read.  window: [1024] fp32, DEVICE memory, the periodic Hann window of efts_denoise.  Frames:
 * those of efts_denoise, T = 1 + len / 256 when len > 512 and none otherwise, centred, reflected without edge repeat; frames 2 p and 2 p + 1
 * of an item share one complex transform (frame 2 p the real part, an unpaired last frame has a zero partner), and the magnitude of a bin is
 * m = sqrtf(fma(re, re, im * im)): the same instructions in both entries and in efts_denoise, so all three see the same bits.
 * efts_noise_profile:
 *   energy  : v = fl32(w[n] * x_t[n]); e[t] = sum_n (double) v * (double) v (every product is exact in float64).  ONE order: lane l of 64 starts
 *             from 0 and takes n = l, l + 64, .., l + 960 in ascending order, then v = v + (the v of the lane 32 across), then 16, 8, 4, 2, 1.
 *   noise frames: e_max = max_t e[t]; r = 10^(top_db / 10), computed by the caller in float64 and passed by value (as efts_trim's); frame t is
 *             a noise frame iff e[t] * r < e_max -- one float64 multiply, one strict compare, no logarithm.  K = their count.  An all-zero
 *             item has none.
 *   profile : profile[b][f] = (float) (S[f] / (double) K), f = 0 .. 512, where S[f] is the float64 sum of m[t][f] over the noise frames: the
 *             item's frames are cut into runs of 16 (run q = frames 16 q .. 16 q + 15); every run adds its noise frames from 0 in
 *             ascending t; the runs' sums are added from 0 in ascending q (a run without a noise frame adds nothing).  Rounded once.
 *             K < min_frames (by value, >= 1), or no frame at all: the row is exactly 0.0f and noise_frames still says K.  Entries of a row
 *             behind 512 are not touched.
 *   noise_frames [B], frames [B] int32: K and T.  noise_db [B] float64: 10 log10((sum of e over the noise frames / K) / e_max), NaN for
 *             K = 0; the sum: thread t of 256 adds its noise frames among t, t + 256, .. in ascending order, the xor tree above inside each
 *             wave, then ((wave 0 + wave 1) + wave 2) + wave 3.  Informational: no decision depends on it.
 *   Four launches on one stream whatever the data: the energies (one wave per frame); per item e_max, the flags and the counts; the
 *   transforms of the pairs that hold a noise frame (one wave per run, the sums in registers, one partial row per run to the workspace); the
 *   sum over the runs.  No spectrogram in memory, no atomics, no launch geometry from device data, nothing read back: the call can be
 *   captured.  An item gives the same bits alone, at any batch position and whatever lies behind its samples.
 *   workspace: efts_noise_profile_workspace_bytes(B, max_len) bytes, 16-byte aligned (energies and flags [B][T_max], T_max = 1 + max_len / 256,
 *   counts and partial rows [B][ceil(T_max / 16)][513] float64); contents afterwards unspecified.  The size entry returns 0 for a B or max_len
 *   that the call refuses.
 * efts_spectral_gate: efts_denoise, to the letter (pairing, runs of 16 hops, overlap-add oldest first, one division, zeros behind len up to
 *   ld_out, items of at most 512 samples copied, frames [B] = T), with four differences:
 *   (a) profile [B][ld_profile] fp32, DEVICE memory, row b for item b; ld_profile = 0: one shared row [513] (efts_denoise's bias).
 *   (b) d = m - strength * profile[b][f]; g = d / m if d > 0, otherwise 0; then g = max(g, floor), 0 <= floor <= 1 by value; X' = g X (0
 *       where m = 0).  The zero partner of an unpaired last frame keeps gain 0.  floor = 0 on fp32 samples with a shared row gives the bits
 *       of efts_denoise.
 *   (c) int16 input as above; out is always fp32.
 *   (d) bypass [B] int32, DEVICE memory, may be NULL: a non-zero entry copies the item's samples (int16: fl32((float) sample * pcm_scale))
 *       to out bit for bit, as an item of at most 512 samples is copied; frames[b] is still T.
 *   One launch, no workspace, no atomics, nothing read back.
 * EFTS_EINVAL, nothing launched, the entry's name in efts_last_error(): a null pointer (other than bypass) or one not aligned to its element
 * (the workspace: to 16 bytes), B outside 1 .. 65535, max_len outside 1 .. 2^31 - 8193, a leading dimension below max_len, ld_out >= 2^31,
 * ld_profile below 513 (the gate: other than 0 and below 513), a negative or non-finite strength, a floor outside 0 .. 1, r not a finite
 * number > 1, min_frames < 1, pcm_scale not a positive number with pcm16, a workspace too small, out [B][ld_out] overlapping audio.
 * ---------------------------------------------------------------------------------- */
int64_t efts_noise_profile_workspace_bytes(int32_t B, int32_t max_len);
int efts_noise_profile(const void* audio, int32_t pcm16, float pcm_scale, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window,
                       double r, int32_t min_frames, float* profile, int64_t ld_profile, int32_t* noise_frames, int32_t* frames, double* noise_db,
                       void* workspace, int64_t workspace_bytes, int32_t B, void* stream);
int efts_spectral_gate(const void* audio, int32_t pcm16, float pcm_scale, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window,
                       const float* profile, int64_t ld_profile, float strength, float floor, const int32_t* bypass, float* out, int64_t ld_out,
                       int32_t* frames, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * True-peak metering after ITU-R BS.1770 Annex 2 / EBU R 128 (4x oversampling) of a padded batch, and a look-ahead peak limiter that holds
 * every item under a true-peak ceiling.  Samples fp32, or int16 PCM on the _pcm16 entries, taken as x = fl32((float) sample * pcm_scale)
 * (pcm_scale = 1 / max_wav_value) at the load.  Item b is row b of in [B][ld_in] with len = lengths[b], clamped to 0 .. ld_in; x = 0 outside
 * [0, len); nothing at or behind len is read.
 *   interpolator: table, HOST memory, [4][25] fp32, read during the call: a 4-phase Kaiser-windowed sinc at the Nyquist cutoff with 12 zero
 *               crossings per side and beta = 8.  With t = q / 4 - k for q = 0 .. 3 and k = -12 .. 12:
 *               h[q][k + 12] = sinc(t) I0(8 sqrt(1 - (t / 12)^2)) / I0(8) for |t| < 12 and 0 otherwise, sinc(t) = sin(pi t) / (pi t),
 *               sinc(0) = 1 and sinc of any other integer EXACTLY 0, built in float64 by the caller and rounded once to fp32.  Phase 0 is
 *               therefore the identity to the bit (h[0][12] = 1, every other entry +0.0); a table whose phase 0 is anything else is refused.
 *   oversampled : xo[i][q] = sum over k = -12 .. 12 of x[i + k] h[q][k + 12]: fp32, acc = fmaf(x[i + k], h[q][k + 12], acc) from +0.0 in
 *               ascending k, for q = 1 .. 3; xo[i][0] = x[i].  p[i] = max over q of |xo[i][q]| (a maximum has no order).  As
 *               p[i] >= |x[i]|, true peak >= sample peak holds exactly.
 * efts_true_peak / efts_true_peak_pcm16:
 *   true_peak[b] = max of p[i] and sample_peak[b] = max of |x[i]| over i = 0 .. len - 1, both fp32, both 0 for an empty item.
 * efts_peak_limit / efts_peak_limit_pcm16, with the ceiling c > 0 by value, hold H and smooth S, 1 <= S <= H <= EFTS_LIMITER_MAX_HOLD:
 *   needed gain: r[i] = c / p[i] (one fp32 division, rounded to nearest) if p[i] > c, otherwise 1; r[i] = 1 for i outside [0, len).
 *   hold       : m[i] = min of r[j] over |j - i| <= H.
 *   smoothing  : g[i] = min(r[i], s[i] / (float) (2 S + 1)), s[i] = the m[j] with |j - i| <= S added in fp32 from +0.0 in ascending j,
 *               one fp32 division.  S <= H makes every m[j] of the mean <= r[i], so g <= r and |x[i] g[i]| <= c in real arithmetic; in fp32
 *               the division and the product round once each: |out[i]| <= c (1 + 2^-23).
 *   out[b * ld_out + i] = x[i] * g[i] for i < len and +0.0 for len <= i < ld_out.  Where every p <= c, every g is exactly 1 and the item
 *               comes back bit for bit.
 *   gain_min[b] (fp32) = min of g[i], limited[b] (int32) = the count of g[i] < 1, true_peak[b] (fp32) = max of p[i], all over i < len; an
 *               empty item has 1, 0 and 0.
 *   What bounds the TRUE peak of the output is how smooth g is: the sample peak is bounded as above, the signal between the samples of the
 *   output only as far as g moves little over the interpolator's 25 taps.
 * Two launches each, whatever the data.  A workgroup owns a chunk of EFTS_LIMITER_CHUNK samples, chunk origins at multiples of the chunk
 * size from the item's start, stages it with its halo (12 samples per side; the limiter: 12 + H + S) and writes one partial (16 bytes) per
 * chunk; p, r, m and g never leave the workgroup.  The second launch takes the maximum, the minimum and the integer sum of the partials per
 * item.  No atomics, nothing read back, no launch geometry from device data: the calls can be captured.  An item gives the same bits alone,
 * at any batch position, in any run and whatever lies behind its samples.
 * workspace : device memory, 16-byte aligned, efts_limiter_workspace_bytes(B, max_len = ld_in) bytes: [B][ceil(ld_in / CHUNK)] partials.
 *             Contents afterwards: unspecified.  The size entry returns 0 for arguments the calls would refuse.
 * EFTS_ESHAPE, nothing launched: B outside 1 .. 65535, ld_in outside 1 .. 2^31 - 8193, ld_out below ld_in or above 2^31 - 8193, H or S
 * outside 1 <= S <= H <= EFTS_LIMITER_MAX_HOLD.  EFTS_EINVAL: a null pointer, a pointer not aligned to its element (the workspace: to 16
 * bytes), a table entry that is not finite or a phase 0 that is not the identity, a ceiling that is not a finite number > 0, pcm_scale not a
 * positive number, out [B][ld_out] overlapping in (a chunk reads its neighbours' samples: the limiter does not work in place).
 * ---------------------------------------------------------------------------------- */
#define EFTS_LIMITER_CHUNK 2048
#define EFTS_LIMITER_MAX_HOLD 128
int64_t efts_limiter_workspace_bytes(int32_t B, int64_t max_len);
int efts_true_peak(const float* in, int64_t ld_in, const int32_t* lengths, const float* table, float* true_peak, float* sample_peak, void* workspace,
                   int32_t B, void* stream);
int efts_true_peak_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, const float* table, float pcm_scale, float* true_peak,
                         float* sample_peak, void* workspace, int32_t B, void* stream);
int efts_peak_limit(const float* in, int64_t ld_in, const int32_t* lengths, const float* table, float ceiling, int32_t hold, int32_t smooth, float* out,
                    int64_t ld_out, float* gain_min, int32_t* limited, float* true_peak, void* workspace, int32_t B, void* stream);
int efts_peak_limit_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, const float* table, float pcm_scale, float ceiling, int32_t hold,
                          int32_t smooth, float* out, int64_t ld_out, float* gain_min, int32_t* limited, float* true_peak, void* workspace, int32_t B,
                          void* stream);

/* ------------------------------------------------------------------------------------
 * IIR filtering of a padded batch: a cascade of K second-order sections, 1 <= K <= EFTS_IIR_MAX_SECTIONS, in fp64 with the exact filter
 * state carried from segment to segment.  Samples fp32, or int16 PCM on the _pcm16 entry, taken as x = fl32((float) sample * pcm_scale)
 * (pcm_scale = 1 / max_wav_value) at the load and widened to fp64 without rounding.  Item b is row b of in [B][ld_in] with len =
 * lengths[b], clamped to 0 .. ld_in; nothing at or behind len is read.
 *   filter     : sos, HOST memory, double [K][5], read during the call: (b0, b1, b2, a1, a2) of every section, a0 = 1.  A first-order section
 *                has b2 = a2 = 0.  Every section must satisfy |a2| < 1 and |a1| < 1 + a2 (both poles inside the unit circle).
 *   recurrence : the sections run in order on every sample, section q on the y of section q - 1, each in transposed direct form II with
 *                every product folded into an fma:
 *                    y  = fma(b0, x, s1)
 *                    s1 = fma(-a1, y, fma(b1, x, s2))
 *                    s2 = fma(-a2, y, b2 * x)
 *                Every item starts from s1 = s2 = 0 in every section at its sample 0.  In real arithmetic this is y = b0 x + s1,
 *                s1 = b1 x - a1 y + s2, s2 = b2 x - a2 y.
 *   output     : out[b * ld_out + i] = fl32(y of the last section at sample i) for i < len, one rounding, and +0.0 for len <= i < ld_out.
 * State carry.  S = (s1, s2 of section 0, s1, s2 of section 1, ...) is the cascade's state, N = 2 K doubles.  The segments of an item are
 * its samples [s L, (s + 1) L) with L = EFTS_IIR_SEGMENT, counted from its sample 0.  Over a segment S_end = M S_start + Z: Z is the end
 * state of the run from zero state over the segment's samples, M the N x N matrix whose column i is the end state after L steps with x = 0
 * from the unit state e_i.
 *   powers     : DEVICE memory, double [6][N][N] row-major, read by launch B: M^(2^k) for k = 0 .. 5, entry [k] being the end states after
 *                2^k L zero-input steps of the recurrence above, built by the caller in float64 (numpy has no fma: it runs the real-arithmetic
 *                form, rounding every operation).
 *   launch A   : one thread per segment s with (s + 1) L < len (a full segment that has a successor) computes Z_s by the recurrence.
 *   launch B   : one wave per item takes the segments 64 at a time, lane l on segment c + l of the chunk that begins at segment c, and keeps
 *                P, the end state of its segment.  With C the state at the chunk's start (0 for the first chunk):
 *                    P_l = Z_(c + l), or 0 where launch A wrote none;
 *                    lane 0: P_0[i] = the chain acc = P_0[i], acc = fma(M[i][j], C[j], acc) for j = 0 .. N - 1 ascending;
 *                    for k = 0 .. 5 in turn, every lane l >= 2^k at once from the values before the step:
 *                        P_l[i] = the chain acc = P_l[i], acc = fma(M^(2^k)[i][j], P_(l - 2^k)[j], acc) for j ascending;
 *                    the start state of segment c + l is P_(l - 1), and C for lane 0; the next chunk's C is P_63.
 *   launch C   : one thread per segment runs the recurrence from its start state over its samples and writes the output.
 * The result differs from the sample-by-sample run from sample 0 only by the fp64 rounding of this reassociation.  Three launches, whatever
 * the data: no atomics, nothing read back, no launch geometry from device data, so the calls can be captured.  The segment grid is per item,
 * so an item gives the same bits alone, at any batch position, in any run and whatever lies behind its samples.
 * workspace : device memory, 16-byte aligned, efts_iir_workspace_bytes(B, max_len = ld_in) bytes: [B][ceil(ld_in / L)] slots of 8 doubles.
 *             Contents afterwards: unspecified.  The size entry returns 0 for arguments the calls would refuse.
 * EFTS_ESHAPE, nothing launched: B outside 1 .. 65535, ld_in outside 1 .. 2^31 - 8193, ld_out below ld_in or above 2^31 - 8193, sections
 * outside 1 .. EFTS_IIR_MAX_SECTIONS.  EFTS_EINVAL: a null pointer, a pointer not aligned to its element (the workspace: to 16 bytes), a
 * coefficient that is not finite, a section with a pole on or outside the unit circle, pcm_scale not a positive number,
 * out [B][ld_out] overlapping in (the input is read twice: the filter does not work in place).
 * ---------------------------------------------------------------------------------- */
#define EFTS_IIR_SEGMENT 256
#define EFTS_IIR_MAX_SECTIONS 4
int64_t efts_iir_workspace_bytes(int32_t B, int64_t max_len);
int efts_iir(const float* in, int64_t ld_in, const int32_t* lengths, const double* sos, int32_t sections, const double* powers, float* out,
             int64_t ld_out, void* workspace, int32_t B, void* stream);
int efts_iir_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, const double* sos, int32_t sections, const double* powers,
                   float pcm_scale, float* out, int64_t ld_out, void* workspace, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------
 * One HiFi-GAN ResBlock2 (nntts/vocoders/hifigan_model.py:71-93) in ONE launch: two pre-activation turns
 *     x <- x + conv_{k,d}(LeakyReLU(x))
 * with dilations d0 and d1 on a row space of m rows and c channels (channel-last, one row per sample).
 * Inputs : x, the fp32 stream [m][ldx]; p0, the operand plane of LeakyReLU(x) * rowmask as its producer wrote it (format `split`,
 *          row stride ldp bytes, ceil(c / 64) (split 1) or ceil(c / 32) (split 2, 3) chunks per row); w0, w1, the packed weights of the
 *          two convolutions ([k][c][ldw] of efts_pack_weight, format `split`, tap stride w_tap_stride bytes); bias0, bias1 [c] or NULL;
 *          rowmask [m] (or NULL: all ones).
 * With h0 = (k - 1) / 2 * d0, h1 = (k - 1) / 2 * d1 and P(row) = 0 for every row outside 0 .. m - 1 (the zero guard rows: nothing is read
 * there), per row r and column j < c:
 *     a1[r][j] = sum over chunk ascending, tap t = 0 .. k - 1 ascending, k-slice ascending of P0[r + t d0 - h0][.] . W0[t][j][.]
 *                (fp32 accumulation on the MFMA of the format: one mfma_f32_32x32x16_bf16 per 16 k's for split 1; lo*hi, hi*lo, hi*hi
 *                per 16 k's for split 2; v_mfma_f32_32x32x2_f32 in the k order of efts_gemm for split 3)
 *     y1[r][j] = ((a1 + bias0[j]) + x[r][j]) * rowmask[r]                                     -- the epilogue order of efts_gemm
 *     P1[r][j] = the plane value of v = y1 > 0 ? y1 : y1 * slope, rounded as plane_act of efts_gemm rounds: split 1 bf16(v) (nearest
 *                even); split 2 hi = bf16(v), lo = bf16(v - hi); split 3 v itself
 *     a2[r][j] = the same contraction of P1 with W1 at dilation d1
 *     out[r][j] = ((a2 + bias1[j]) + y1[r][j]) * rowmask[r],  fp32 [m][ldo]; columns j >= c of out are not written.
 * y1 and P1 never reach memory: a workgroup owns 32 n - 2 h1 rows (n <= 6 blocks of 32, as many as fit the LDS), stages the window of P0
 * with both halos in LDS, computes y1 on its rows plus the second halo, overwrites the window with P1 and contracts again.  The result of
 * a row depends on the values of rows r - h0 - h1 .. r + h0 + h1 alone, never on where a tile begins: an item gives the same bits alone
 * or anywhere in a batch, and the result equals two efts_gemm launches (plane_act, resid, rowmask) up to the summation order inside the
 * fp32 accumulator.  No atomics, no launch geometry from device data: capturable.
 * EFTS_EINVAL: null args / operand, split outside 1 .. 3, k outside {3, 5, 7, 9, 11}, reserved != 0.  EFTS_ESHAPE: m <= 0, c outside
 * 4 .. 128 or c % 4 != 0, d0 or d1 outside 1 .. 64, (k - 1) / 2 * (d0 + d1) > 64, a row stride below the row.  EFTS_EALIGN: x, p0, w0, w1, out or a row / tap stride
 * not 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
typedef struct efts_resblock2_args {
    const float* x;       /* fp32 [m][ldx] */
    int64_t ldx;          /* elements, % 4 == 0 */
    const void* p0;       /* operand plane of LeakyReLU(x) * rowmask, row 0 */
    int64_t ldp;          /* bytes */
    const void* w0;       /* packed weights of the two convolutions */
    const void* w1;
    int64_t ldw;          /* bytes, both */
    int64_t w_tap_stride; /* bytes, both */
    const float* bias0;   /* [c] or NULL */
    const float* bias1;
    const float* rowmask; /* [m] or NULL */
    float* out;           /* fp32 [m][ldo] */
    int64_t ldo;          /* elements, % 4 == 0 */
    int32_t split;        /* 1, 2 or 3: format of p0, w0, w1 and of the intermediate plane */
    int32_t m;            /* rows */
    int32_t c;            /* channels */
    int32_t k;            /* kernel size of both convolutions */
    int32_t d0, d1;       /* their dilations */
    float slope;          /* LeakyReLU slope of the intermediate */
    int32_t reserved;     /* 0 */
} efts_resblock2_args;
int efts_resblock2(const efts_resblock2_args* a, void* stream);

/* ------------------------------------------------------------------------------------
 * The head of an iSTFTNet generator (Kaneko et al., ICASSP 2022: a HiFi-GAN trunk whose conv_post emits N + 2 channels, a log-magnitude
 * and a phase argument per bin of an N-point STFT, followed by an inverse STFT with hop h = N / 4).  N in {8, 16, 32}.
 * Per item: L rows at the last stage (L = lengths[b] * len_mul; 0 or >= 4), a[m] the C-channel row of leaky_relu(mean, 0.01), m < L.
 *   Reflection pad (1, 0):  a'[0] = a[1], a'[m] = a[m - 1] for m = 1 .. L: the item has L + 1 frames.
 *   Convolution:            z[f][c] = bias[c] + sum_{j = 0 .. 6} W[c][:, j] . a'[f + j - 3], a' = 0 outside 0 .. L, f = 0 .. L, c = 0 .. N + 1.
 *                           (an efts_gemm launch of 7 taps on the plane of a', n = N + 2, fp32 output with ldo = N + 2, no activation, a row
 *                           mask over the L + 1 frames: the operand rounding of the three formats is that launch's)
 *   Spectrum, K = N / 2 + 1, k < K:  mag = exp(z[f][k]), ph = sin(z[f][K + k]), X_f[k] = mag * (cos ph + i sin ph); the imaginary
 *                           parts of bins 0 and N / 2 are ignored.
 *   Frame, n < N:           y_f[n] = (1 / N) * ((Re X[0] + (-1)^n Re X[N/2]) + 2 * sum_{k = 1 .. N/2 - 1} (Re X[k] cos(2 pi k n / N) -
 *                           Im X[k] sin(2 pi k n / N))), the sum in ascending k, one fused multiply-add per product, the cosines and
 *                           sines read from `twiddle` at (k n) mod N.
 *   Window:                 w[n] = 0.5 - 0.5 cos(2 pi n / N) (periodic Hann), built by the host in float64 and rounded to fp32: `window`.
 *   Output, 0 <= t < h L:   u = t + N / 2, F(u) = { f : 0 <= f <= L, h f <= u < h f + N },
 *                           out[t] = (sum_{f in F(u)} w[u - h f] * y_f[u - h f]) / (sum_{f in F(u)} w[u - h f]^2), both sums in ascending f
 *                           (at most four terms; the divisor is the true envelope: 1.5 inside, other values in the first and last N / 2
 *                           samples, never 0); out[t] = 0 for h L <= t < out_len.
 * This is torch.istft(mag * exp(1j * ph), N, h, N, window=hann_window(N), center=True) of the published TorchSTFT.inverse.
 *
 * mode EFTS_ISTFT_SYNTH: z fp32 [z_rows][N + 2] (row stride N + 2 exactly) in the row space of the batch, frame f of item b at row
 *   b * pitch + f; lengths int32 [B]; window fp32 [N]; twiddle fp32 [N][2] = (cos, sin)(2 pi j / N); audio fp32 [B][ld_audio], samples
 *   0 .. out_len - 1 of every item are written (out_len % 4 == 0).  One workgroup owns 1024 consecutive samples of one item (1024 / h
 *   frames of hops), stages the frames that touch them (one in front, two behind) with 16-byte loads, turns them into windowed frames
 *   in LDS and overlap-adds from there; 16-byte stores.  L is clipped to out_len / h and to pitch - 1.  Rows of z outside an item's
 *   frames are never used: an item gives the same bits alone, anywhere in a batch and whatever lies behind it.  No atomics, nothing read
 *   back, no launch geometry from device data: capturable.
 * mode EFTS_ISTFT_REFLECT: the reflected row.  plane: row 0 of the operand plane of a (any format, row stride ld_plane bytes, at least one
 *   row in front of row 0); for every item the whole row b * pitch + 1 is copied to row b * pitch - 1, so that a contraction reading
 *   the plane from one row further up sees a'.  (The row lies in the guard rows for item 0 and in the gap rows behind the item in front
 *   for the others; the caller keeps L + 4 <= pitch.)  Only B, pitch, plane and ld_plane are read.
 * EFTS_EINVAL: null args / operand, n_fft outside {8, 16, 32}, hop != n_fft / 4, mode outside 0 .. 1, reserved != 0.  EFTS_ESHAPE: B outside
 * 1 .. 65535, pitch < 4 or odd, len_mul < 1, z_rows < 1, out_len < 4 or % 4 != 0, ld_audio < out_len.  EFTS_EALIGN: z, audio or plane not
 * 16-byte aligned, ld_audio % 4 != 0, ld_plane % 16 != 0.
 * ---------------------------------------------------------------------------------- */
#define EFTS_ISTFT_SYNTH 0
#define EFTS_ISTFT_REFLECT 1
#define EFTS_ISTFT_RUN 1024 /* samples per workgroup */
typedef struct efts_istft_head_args {
    const float* z;         /* fp32 [z_rows][n_fft + 2] */
    const int32_t* lengths; /* [B] */
    const float* window;    /* [n_fft] */
    const float* twiddle;   /* [n_fft][2] */
    float* audio;           /* fp32 [B][ld_audio] */
    int64_t ld_audio;       /* elements, % 4 == 0 */
    void* plane;            /* EFTS_ISTFT_REFLECT: row 0 of the operand plane */
    int64_t ld_plane;       /* bytes, % 16 == 0 */
    int32_t mode;           /* EFTS_ISTFT_SYNTH or EFTS_ISTFT_REFLECT */
    int32_t B;              /* items */
    int32_t pitch;          /* rows per item in the row space, even */
    int32_t z_rows;         /* rows of z that may be read */
    int32_t len_mul;        /* rows per unit of `lengths` */
    int32_t out_len;        /* samples written per item, % 4 == 0 */
    int32_t n_fft;          /* 8, 16 or 32 */
    int32_t hop;            /* n_fft / 4 */
    int32_t reserved;       /* 0 */
    int32_t reserved2;      /* 0 */
} efts_istft_head_args;
int efts_istft_head(const efts_istft_head_args* a, void* stream);

/* ------------------------------------------------------------------------------------
 * BigVGAN's anti-aliased periodic activation (Lee et al., ICLR 2023: Activation1d around Snake / SnakeBeta) in ONE launch: upsample by 2
 * with a 12-tap Kaiser-windowed sinc, v = u + inv_b sin(a u)^2 per channel, low-pass and downsample by 2 with the same filter, replicate
 * padding at both ends of every item.
 * Filter: f[k] = 0.5 w[k] sinc(0.5 (k - 5.5)) normalised to sum 1, w = the symmetric Kaiser window of 12 points with beta = 0.1102 (A - 8.7),
 *   A = 2.285 * 5 * pi * 1.2 + 7.95 (cutoff 0.25, half-width 0.3); built in float64, rounded once to fp32, compiled into the kernel.
 *   f[11 - k] = f[k]; f[0 .. 5] = 0.0020289664498962423, 0.00938946394406788, -0.02554346406529466, -0.05765737547536495,
 *   0.12857260908132875, 0.4432098000653667.
 * Per item b: L = clamp(lengths[b], 0, T) * len_mul rows at rows b * pitch .. b * pitch + L - 1 of x, per channel j < c, with
 * X(i) = x[clamp(i, 0, L - 1)][j]:
 *   2x-rate sample m, taken at m' = clamp(m, 0, 2L - 1), with i0 = m' >> 1:
 *     m' even:  u = 2 * sum_{i = 0 .. 5} f[2i + 1] * X(i0 + 2 - i)
 *     m' odd :  u = 2 * sum_{i = 0 .. 5} f[2i]     * X(i0 + 3 - i)        both sums from 0 in ascending i, one fused multiply-add per term
 *     v(m) = fma(inv_b[j], s * s, u),  s = sinf(a[j] * u)                  (the product rounded to fp32, the accurate sinf)
 *   y[t] = sum_{k = 0 .. 11} f[k] * v(2t + k - 5),  t < L                  from 0 in ascending k, one fused multiply-add per term
 *   y[t] = 0 for L <= t < T * len_mul.  y[t] depends on x[t - 5 .. t + 5] of its own item alone.
 * Outputs, either or both: `out` fp32 [.][ldo] and `plane`, the operand plane of y in format `split`, rounded as plane_act of efts_gemm
 * rounds (split 1 bf16(y), nearest even; split 2 hi = bf16(y), lo = bf16(y - hi); split 3 y itself).  Rows b * pitch .. b * pitch +
 * T * len_mul - 1 of every item are written, columns 0 .. c - 1 of out and every column of the plane's chunks (c .. roundup(c, 64 or 32) - 1
 * as zeros); the rows between items, guard rows and columns past c of out are not touched.
 * One lane owns 4 adjacent channels and EFTS_SNAKE_SEG consecutive rows of one item and walks down them with the 6 rows of x of one pair of
 * 2x-rate samples and the 12 values of v of one output row in registers; a segment recomputes the 10 values in front of its first row.
 * No LDS, no barrier, no atomics, nothing read back, no launch geometry from device data: capturable.  An item gives the same bits alone,
 * anywhere in a batch and whatever lies behind it.
 * a and inv_b are made by the host in float64 from the fp32 parameters and rounded once: a = exp(alpha) (snake_logscale) or alpha;
 * inv_b = 1 / (a + 1e-9) (Snake) or 1 / (b + 1e-9) with b from beta the same way (SnakeBeta).
 * EFTS_EINVAL: null args / x / lengths / a / inv_b, neither plane nor out, split outside 1 .. 3 with a plane, reserved != 0.  EFTS_ESHAPE: c < 4 or
 * c % 4 != 0, B outside 1 .. 65535, T, len_mul or pitch < 1, T * len_mul > pitch, B * pitch > 2^31 - 1, a row stride below the row.
 * EFTS_EALIGN: x, a, inv_b, out or plane not 16-byte aligned, ldx % 4, ldo % 4 or ld_plane % 16 != 0, lengths not 4-byte aligned.
 * ---------------------------------------------------------------------------------- */
#ifndef EFTS_SNAKE_SEG
#define EFTS_SNAKE_SEG 32 /* rows per lane */
#endif
typedef struct efts_snake_aa_args {
    const float* x;         /* fp32 [B * pitch][ldx] */
    int64_t ldx;            /* elements, % 4 == 0 */
    const int32_t* lengths; /* [B] */
    const float* a;         /* [c] */
    const float* inv_b;     /* [c] */
    void* plane;            /* operand plane of the result, row 0, or NULL */
    int64_t ld_plane;       /* bytes, % 16 == 0 */
    float* out;             /* fp32 [B * pitch][ldo], or NULL */
    int64_t ldo;            /* elements, % 4 == 0 */
    int32_t split;          /* 1, 2 or 3: format of the plane */
    int32_t B;              /* items */
    int32_t pitch;          /* rows per item in the row space */
    int32_t T;              /* units of `lengths` per item at the most: T * len_mul rows of every item are written */
    int32_t len_mul;        /* rows per unit of `lengths` */
    int32_t c;              /* channels, % 4 == 0 */
    int32_t reserved;       /* 0 */
    int32_t reserved2;      /* 0 */
} efts_snake_aa_args;
int efts_snake_aa(const efts_snake_aa_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EFTS_ABI_H */
