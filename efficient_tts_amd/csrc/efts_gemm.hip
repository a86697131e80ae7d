// efts_gemm.hip -- the MFMA contraction of the EFTS-CNN path on gfx950 (CDNA4).
//
//   out[row, col] = epi( alpha * sum_{tap} sum_{k} A[row + tap - pad, k] * Bw[tap][col, k] )
//
// One kernel serves the residual Conv1d stacks (taps 5; reference
// nntts/layers/efts_modules.py:48-51), the duration-predictor convs (taps 3;
// nntts/layers/duration_predictor.py:57), the Linears (taps 1; efficient_tts.py:149-153,161,198)
// and the two batched matrix products of the alignment block (efficient_tts.py:190,390).
//
// Design (MI355X-first):
//   * activations are channel-last in a padded row space, so a k-tap convolution is a GEMM
//     whose A tile is ONE 128-row LDS window read at `taps` row shifts: the window is staged
//     once per K-chunk and re-used by every tap (LDS-staged conv window).  A tile therefore
//     produces 128 - (taps - 1) output rows (124 for k5): the window is exactly 16 KiB, and
//     2 windows + a 3-stage weight ring are exactly 80 KiB = two workgroups per CU.
//   * 256-thread workgroup, 2x2 waves of 64x64, 32x32x16 bf16 MFMA, fp32 accumulators (efts_gemm_ring.h; narrower column
//     tiles re-split the waves, see there).
//   * operands arrive by LDS-DMA (global_load_lds_dwordx4, 16 B/lane), issued from inline asm with
//     a scalar base + a per-lane 32-bit offset computed once per tile.  (Issued through the clang
//     builtin, hipcc cannot prove that a window read does not alias an in-flight DMA and puts an
//     s_waitcnt vmcnt(0) in front of the ds_reads of every step, which serialises the pipeline.)
//     The weight tile of step s+2 is in flight while step s computes; steps end with a COUNTED
//     s_waitcnt vmcnt(N) + s_barrier.  The LDS image is lane-linear, so the bank-conflict swizzle is
//     applied on the per-lane SOURCE address and again on the ds_read_b128 address.
//   * K is consumed in 128-byte chunks: 64 bf16 ("bf16"), or 32 hi + 32 lo bf16 ("bf16x3":
//     x = hi + lo, product = hi*hi + hi*lo + lo*hi, fp32 accumulate -> fp32-class accuracy at
//     3 MFMAs per product instead of the 16x slower f32 MFMA), or 32 fp32 ("fp32", split 3: the exact
//     operands on v_mfma_f32_32x32x2_f32, generic tiling only -- the reference-parity mode).
//   * epilogue fused: bias, LeakyReLU/ReLU, residual add, row mask (gap rows / padded
//     positions), fp32 store and bf16 operand planes for the next contraction.  The residual and
//     mask values are requested at the start of the LAST K step, so their HBM latency hides under
//     that step and the LDS staging of the accumulators; stores are never waited for (efts_gemm_epilogue.h, shared by all tilings).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "efts_gemm_ring.h"   // gemm_kernel: this file instantiates the 128-column tiles (efts_gemm_narrow.hip the 64- / 32-column ones)

using namespace efts;

template <int T, int S, int D>
static void launch_one(dim3 grid, hipStream_t st, const GemmKernelArgs& k) {
    if (D) (void)hipFuncSetAttribute((const void*)gemm_kernel<T, S, BN, D>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS);
    hipLaunchKernelGGL((gemm_kernel<T, S, BN, D>), grid, dim3(256), GEMM_LDS, st, k);
}

#ifdef EFTS_LAB
// Lab builds: debug instantiation (k5 only) honouring EFTS_GEMM_DBG ablation bits and, with EFTS_GEMM_PROF=1, printing
// per-phase s_memtime sums of every wave.  Synchronises the stream.
template <int S>
static void launch_debug(dim3 grid, hipStream_t st, GemmKernelArgs k, int prof) {
    static unsigned long long* buf = nullptr;
    if (prof) {
        if (!buf) (void)hipMalloc((void**)&buf, 64);
        (void)hipMemsetAsync(buf, 0, 64, st);
        k.prof = buf;
    }
    if (prof) launch_one<5, S, 2>(grid, st, k); else launch_one<5, S, 1>(grid, st, k);
    if (prof) {
        unsigned long long h[8];
        (void)hipMemcpyAsync(h, buf, 56, hipMemcpyDeviceToHost, st);
        (void)hipStreamSynchronize(st);
        const double w = (double)h[6];
        fprintf(stderr, "[efts prof] waves %.0f  per-wave cycles: issue %.0f  mfma+reads %.0f  dma-wait %.0f  barrier %.0f  epilogue %.0f\n",
                w, h[0] / w, h[2] / w, h[3] / w, h[4] / w, h[5] / w);
    }
}
#endif

extern "C" int efts_gemm(const efts_gemm_args* a, void* stream) {
    if (!a) return efts_fail(EFTS_EINVAL, "efts_gemm: null args");
    if (!(a->split >= EFTS_SPLIT_BF16 && a->split <= EFTS_SPLIT_FP32)) return efts_fail(EFTS_EINVAL, "efts_gemm: split must be 1, 2 or 3");
    if (!(a->taps == 1 || a->taps == 3 || a->taps == 5 || a->taps == 7 || a->taps == 9 || a->taps == 11)) return efts_fail(EFTS_EINVAL, "efts_gemm: taps must be 1, 3, 5, 7, 9 or 11");
    const int dil = a->dilation > 0 ? a->dilation : 1;
    if ((a->taps - 1) * dil > 64) return efts_fail(EFTS_ESHAPE, "efts_gemm: (taps - 1) * dilation must not exceed 64 rows");
    if (a->m <= 0 || a->n <= 0 || a->nchunk <= 0 || a->batch <= 0) return efts_fail(EFTS_ESHAPE, "efts_gemm: m, n, nchunk, batch must be positive");
    if (!a->a || !a->b) return efts_fail(EFTS_EINVAL, "efts_gemm: null operand");
    if (((uintptr_t)a->a & 15) || ((uintptr_t)a->b & 15) || (a->lda & 15) || (a->ldb & 15) || (a->b_tap_stride & 15) ||
        (a->a_batch_stride & 15) || (a->b_batch_stride & 15))
        return efts_fail(EFTS_EALIGN, "efts_gemm: operand planes must be 16-byte aligned (pointer, row, tap and batch strides)");
    if (a->lda < (int64_t)a->nchunk * 128 || a->ldb < (int64_t)a->nchunk * 128)
        return efts_fail(EFTS_ESHAPE, "efts_gemm: row stride smaller than nchunk*128 bytes");
    if (a->lda > (1 << 23) || a->ldb > (1 << 23)) return efts_fail(EFTS_ESHAPE, "efts_gemm: row stride above 8 MiB");
    if (a->out_bf16 && !(a->out_split >= EFTS_SPLIT_BF16 && a->out_split <= EFTS_SPLIT_FP32)) return efts_fail(EFTS_EINVAL, "efts_gemm: out_split must be 1, 2 or 3");
    if (a->out_bf16 && ((a->out_split == EFTS_SPLIT_FP32) != (a->split == EFTS_SPLIT_FP32)))
        return efts_fail(EFTS_EINVAL, "efts_gemm: out_split 3 (fp32 plane) goes with split 3 operands, and split 3 writes fp32 planes only");
    if (!a->out_f32 && !a->out_bf16 && !a->soft_index) return efts_fail(EFTS_EINVAL, "efts_gemm: no output");

    GemmKernelArgs k;
    k.a = (const char*)a->a; k.b = (const char*)a->b;
    k.bias = a->bias; k.resid = a->resid; k.rowmask = a->rowmask;
    k.out_f32 = a->out_f32; k.out_bf16 = (char*)a->out_bf16; k.out_lo = (char*)a->out_bf16_lo; k.sign = (char*)a->sign_mask;
    k.sidx = a->soft_index; k.klen = a->key_len; k.qlen = a->query_len;
    k.sqerr = a->sqerr_part;
    k.drop_thresh = 0; k.drop_seed_h = 0; k.drop_inv_keep = 1.f;
    if (a->drop_p > 0.f) {
        if (!(a->drop_p < 1.f)) return efts_fail(EFTS_EINVAL, "efts_gemm: drop_p must be in [0, 1)");
        k.drop_thresh = (unsigned)((double)a->drop_p * 4294967296.0);
        k.drop_seed_h = hash_u32(a->drop_seed);
        k.drop_inv_keep = 1.f / (1.f - a->drop_p);
    }
    if (a->out_bf16_lo && (!a->out_bf16 || a->out_split != 1 || a->plane_act || ((uintptr_t)a->out_bf16_lo & 7)))
        return efts_fail(EFTS_EINVAL, "efts_gemm: out_bf16_lo goes with an un-activated split-1 out_bf16 plane (8-byte aligned)");
    k.lda = a->lda; k.ldb = a->ldb; k.b_tap_stride = a->b_tap_stride; k.ldr = a->ldr; k.ldo = a->ldo; k.ldob = a->ldob;
    k.a_bs = a->a_batch_stride; k.b_bs = a->b_batch_stride; k.r_bs = a->resid_batch_stride;
    k.m_bs = a->rowmask_batch_stride; k.o_bs = a->out_batch_stride; k.ob_bs = a->outb_batch_stride;
    k.a_bs2 = a->a_batch2_stride; k.b_bs2 = a->b_batch2_stride; k.o_bs2 = a->out_batch2_stride;
    const int nb2 = a->batch2 > 1 ? a->batch2 : 1;
    if (nb2 > 1 && (a->out_bf16 || a->resid || a->rowmask)) return efts_fail(EFTS_EINVAL, "efts_gemm: batch2 supports fp32 output only");
    k.m = a->m; k.n = a->n; k.nchunk = a->nchunk; k.pad = (a->taps - 1) / 2;
    const int bm = WIN - (a->taps - 1) * dil;
    k.dil = dil; k.bm = bm; k.plane_act = a->plane_act; k.plane_slope = a->plane_slope;
    k.mtiles = (a->m + bm - 1) / bm;
    k.ntiles = (a->n + BN - 1) / BN;
    k.alpha = a->alpha; k.slope = a->slope; k.act = a->act; k.out_split = a->out_split;
    k.vec_ok = (!a->out_f32 || ((a->ldo & 3) == 0 && ((uintptr_t)a->out_f32 & 15) == 0 && (a->out_batch_stride & 3) == 0)) &&
               (!a->resid || ((a->ldr & 3) == 0 && ((uintptr_t)a->resid & 15) == 0 && (a->resid_batch_stride & 3) == 0)) &&
               (!a->out_bf16 || ((a->ldob & 7) == 0 && ((uintptr_t)a->out_bf16 & 7) == 0 && (a->outb_batch_stride & 7) == 0)) &&
               (!a->out_bf16 || a->out_split != EFTS_SPLIT_FP32 || ((a->ldob & 15) == 0 && ((uintptr_t)a->out_bf16 & 15) == 0 && (a->outb_batch_stride & 15) == 0));
    k.prof = nullptr; k.dbg = 0;
    if (a->soft_index && (!a->key_len || !a->query_len || a->n > BN || nb2 > 1 || a->resid || a->out_bf16 || a->taps != 1 || a->act != EFTS_ACT_NONE))
        return efts_fail(EFTS_EINVAL, "efts_gemm: soft_index needs key_len / query_len, n <= 128, one tap, no activation, residual, plane output or batch2");
    if (k.drop_thresh && (a->batch > 1 || nb2 > 1 || !k.vec_ok || a->n % 4 || (long)a->m * a->n > 0xffffffffL))
        return efts_fail(EFTS_EINVAL, "efts_gemm: dropout needs batch 1, 16-byte aligned fp32 / plane rows, n % 4 == 0 and m * n < 2^32");
    if (a->sign_mask && (a->n % 128 || a->batch > 1 || nb2 > 1 || !k.vec_ok || ((uintptr_t)a->sign_mask & 15)))
        return efts_fail(EFTS_EINVAL, "efts_gemm: sign_mask needs n %% 128 == 0, batch 1, 16-byte aligned output rows and mask");
    if (a->sqerr_part) {
        if (!a->sqerr_target || !a->rowmask || a->resid || a->taps != 1 || a->n > BN || (a->n & 3) || nb2 > 1 || k.drop_thresh || a->out_bf16 || a->soft_index ||
            (a->ld_target & 3) || (a->target_batch_stride & 3) || ((uintptr_t)a->sqerr_target & 15) || !k.vec_ok)
            return efts_fail(EFTS_EINVAL, "efts_gemm: sqerr_part needs sqerr_target (16-byte aligned rows), rowmask, one tap, n <= 128, n %% 4 == 0, fp32 output only, no residual / dropout / batch2");
        if (a->tiling > EFTS_TILING_GENERIC) return efts_fail(EFTS_EINVAL, "efts_gemm: sqerr_part needs the generic tiling");
        k.resid = a->sqerr_target; k.ldr = a->ld_target; k.r_bs = a->target_batch_stride;      // the target travels where the residual would
    }
    hipStream_t st = (hipStream_t)stream;

    // ---- which kernel.  `tiling` AUTO (0) applies the measured rules below; the explicit values exist for A/B runs and
    // for the bit-equality tests between the kernels (they all compute identical results).
    const int tiling = a->tiling;
    if (tiling < EFTS_TILING_AUTO || tiling > EFTS_TILING_SMALLM) return efts_fail(EFTS_EINVAL, "efts_gemm: unknown tiling %d", tiling);
    // fp32 planes: the generic kernel only (AUTO goes there); the other tilings have no split-3 main loop and never run one as bf16
    const bool fp32 = a->split == EFTS_SPLIT_FP32;
    if (fp32 && tiling > EFTS_TILING_GENERIC)
        return efts_fail(EFTS_EINVAL, "efts_gemm: split 3 (fp32) runs on the generic tiling only (tiling %d requested)", tiling);
    // train-mode dropout: EPI_DROP exists in the 128-column ring tiles and conv5_kernel only (AUTO keeps such a launch there: `no_narrow`)
    if (k.drop_thresh && tiling > EFTS_TILING_WIDE)
        return efts_fail(EFTS_EINVAL, "efts_gemm: dropout needs the generic or wide tiling (tiling %d requested)", tiling);
    // (0) short row spaces on request (never AUTO: the K dimension is split across the waves, so the summation order -- not the
    //     operand rounding -- differs from the ring kernels): 64 x 32 tiles, fragments straight from global memory
    if (tiling == EFTS_TILING_SMALLM) {
        if (a->batch != 1 || nb2 != 1 || dil != 1 || !(a->taps == 1 || a->taps == 3 || a->taps == 5) || a->n % 32 || a->plane_act || a->act == EFTS_ACT_TANH ||
            a->out_bf16_lo || a->sign_mask || a->soft_index || k.drop_thresh || !k.vec_ok || (a->out_bf16 && ((a->ldob & 15) || ((uintptr_t)a->out_bf16 & 15))) ||
            (a->ldo & 3) || (a->ldr & 3) || a->n % 8)
            return efts_fail(EFTS_ESHAPE, "efts_gemm: the small-M tiling takes one dense 1 / 3 / 5-tap launch, n %% 32 == 0, 16-byte aligned rows, plain outputs");
        if (launch_smallm_any(a->split, a->taps, st, k)) return efts_check_launch("efts_gemm");
        return efts_fail(EFTS_ESHAPE, "efts_gemm: no small-M instantiation for taps %d", a->taps);
    }
    const bool generic_only = a->out_bf16_lo != nullptr || nb2 > 1 || a->soft_index != nullptr || a->sqerr_part != nullptr;      // EPI_LO / EPI_SIDX / EPI_SQERR and the outer batch: the 128-column ring tiles only (ring_features)
    const bool no_narrow = generic_only || a->sign_mask != nullptr || k.drop_thresh != 0;      // EPI_SIGN / EPI_DROP: the 128-column ring tiles and conv5_kernel only
    if (generic_only && tiling > EFTS_TILING_GENERIC) return efts_fail(EFTS_EINVAL, "efts_gemm: out_bf16_lo / batch2 need the generic tiling");
    const dim3 grid(k.mtiles * k.ntiles, a->batch, nb2);                  // one workgroup per 124 x 128 tile, 2 resident per CU

    // (1) one K chunk and at most 64 columns over many rows (the 32- and 64-channel stages of the vocoder): window + all taps
    //     resident in LDS, 32-column tiles (2.11 -> 2.03 ms per utterance, 11.1 -> 10.5 ms per batch of 8)
    const bool resident_ok = a->n <= 64 && a->nchunk == 1 && (a->taps - 1) * dil <= 64 && (a->taps == 3 || a->taps == 7 || a->taps == 11);
    if (tiling == EFTS_TILING_RESIDENT && !resident_ok) return efts_fail(EFTS_ESHAPE, "efts_gemm: the resident tiling needs n <= 64, one K chunk, taps 3 / 7 / 11");
    if (no_narrow && !generic_only && (tiling == EFTS_TILING_NARROW || tiling == EFTS_TILING_RESIDENT))
        return efts_fail(EFTS_EINVAL, "efts_gemm: sign_mask needs the generic or wide tiling");
    if (!fp32 && !no_narrow && resident_ok && (tiling == EFTS_TILING_RESIDENT || (tiling == EFTS_TILING_AUTO && a->m >= 8 * R32_WIN))) {
        GemmKernelArgs kr = k;
        kr.bm = R32_WIN - (a->taps - 1) * dil;
        kr.mtiles = (a->m + kr.bm - 1) / kr.bm;
        kr.ntiles = (a->n + 31) / 32;
        if (launch_resident32_any(a->split, a->taps, dim3(kr.mtiles * kr.ntiles, a->batch, 1), st, kr)) return efts_check_launch("efts_gemm");
    }
    // (2) outputs of at most 64 columns: column tile 64 / 32 -- and launches whose 128-column tiling cannot give every CU one
    //     workgroup (the text side of the acoustic model: 64 x 130 rows = 272 workgroups; the 256-channel stage of the vocoder
    //     at one utterance: 110): such a launch is bound by the per-workgroup step latency, and 64-column tiles double the
    //     number of workgroups that overlap (one per CU is the measured threshold; two was slower for the text side)
    const bool few = (long)k.mtiles * k.ntiles * a->batch < (long)efts_num_cus() && a->n > 64;
    if (!fp32 && !no_narrow && (tiling == EFTS_TILING_NARROW || (tiling == EFTS_TILING_AUTO && (a->n <= 64 || few)))) {
        GemmKernelArgs kn = k;
        kn.ntiles = a->n <= 32 ? 1 : (a->n + 63) / 64;
        if (launch_narrow_any(a->split, a->n <= 32 ? 32 : 64, a->taps, dim3(k.mtiles * kn.ntiles, a->batch, 1), st, kn)) return efts_check_launch("efts_gemm");
        if (tiling == EFTS_TILING_NARROW) return efts_fail(EFTS_ESHAPE, "efts_gemm: no narrow instantiation for taps %d", a->taps);
    }
    // (3) k5 convolutions with at least 400 (252-row tile x column tile) workgroups on bf16 planes: the 256-row kernel
    //     (+1.5 % on the training step's forward / dgrad launches; -2.5 % on bf16x3 planes, hence bf16 only in AUTO).  Its last
    //     window may reach mt5 * 252 + 2 - m rows past the matrix: only inside the 144 guard rows of the ABI.
    const bool wide_ok = a->taps == 5 && dil == 1 && !a->plane_act && a->act != EFTS_ACT_TANH;
    const int mt5 = (a->m + C5_BM - 1) / C5_BM;
    const bool wide_fits = (long)mt5 * C5_BM + 2 - a->m <= 144;
    if (tiling == EFTS_TILING_WIDE && !(wide_ok && wide_fits)) return efts_fail(EFTS_ESHAPE, "efts_gemm: the wide tiling is for dense k5 launches whose last 256-row window stays inside the guard rows");
    if (!fp32 && !generic_only && wide_ok && wide_fits &&
        (tiling == EFTS_TILING_WIDE || (tiling == EFTS_TILING_AUTO && a->split == 1 && (long)mt5 * k.ntiles * a->batch >= C5_DEFAULT_MIN_TILES))) {
        GemmKernelArgs k5 = k;
        k5.mtiles = mt5;
        launch_conv5_any(a->split, dim3(mt5 * k.ntiles, a->batch, 1), st, k5);
        return efts_check_launch("efts_gemm");
    }
#ifdef EFTS_LAB
    {   // lab builds: the 8-wave experiment and the ablation / cycle-stamp instantiations of the generic kernel
        const char* e8 = getenv("EFTS_CONV8");
        if (e8 && atoi(e8) == 1 && wide_ok && wide_fits && a->split == 1 && a->n % C8_BN == 0 && k.vec_ok && !generic_only) {
            GemmKernelArgs k8 = k;
            k8.mtiles = mt5;
            k8.ntiles = a->n / C8_BN;
            launch_conv8(dim3(mt5 * k8.ntiles, a->batch, 1), st, k8);
            return efts_check_launch("efts_gemm");
        }
        const char* ed = getenv("EFTS_GEMM_DBG");
        const char* ep = getenv("EFTS_GEMM_PROF");
        const int dbg = ed ? atoi(ed) : 0, prof = ep ? atoi(ep) : 0;
        if ((dbg || prof) && a->taps == 5 && !fp32) {
            k.dbg = dbg;
            if (a->split == 1) launch_debug<1>(grid, st, k, prof); else launch_debug<2>(grid, st, k, prof);
            return efts_check_launch("efts_gemm");
        }
    }
#endif
    if (fp32) {
        switch (a->taps) {
            case 11: launch_one<11, 3, 0>(grid, st, k); break;
            case 9: launch_one<9, 3, 0>(grid, st, k); break;
            case 7: launch_one<7, 3, 0>(grid, st, k); break;
            case 5: launch_one<5, 3, 0>(grid, st, k); break;
            case 3: launch_one<3, 3, 0>(grid, st, k); break;
            default: launch_one<1, 3, 0>(grid, st, k);
        }
    } else if (a->split == 1) {
        switch (a->taps) {
            case 11: launch_one<11, 1, 0>(grid, st, k); break;
            case 9: launch_one<9, 1, 0>(grid, st, k); break;
            case 7: launch_one<7, 1, 0>(grid, st, k); break;
            case 5: launch_one<5, 1, 0>(grid, st, k); break;
            case 3: launch_one<3, 1, 0>(grid, st, k); break;
            default: launch_one<1, 1, 0>(grid, st, k);
        }
    } else {
        switch (a->taps) {
            case 11: launch_one<11, 2, 0>(grid, st, k); break;
            case 9: launch_one<9, 2, 0>(grid, st, k); break;
            case 7: launch_one<7, 2, 0>(grid, st, k); break;
            case 5: launch_one<5, 2, 0>(grid, st, k); break;
            case 3: launch_one<3, 2, 0>(grid, st, k); break;
            default: launch_one<1, 2, 0>(grid, st, k);
        }
    }
    return efts_check_launch("efts_gemm");
}

// Opt every product instantiation into 80 KiB of dynamic LDS once, at library load.
template <int T, int S>
static void set_lds_attr() {
    (void)hipFuncSetAttribute((const void*)gemm_kernel<T, S, BN, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS);
}
__attribute__((visibility("hidden"))) void efts_gemm_init(void) {
    static bool once = false;
    if (!once) {
        conv5_set_lds_attr();
        set_lds_attr<5, 1>(); set_lds_attr<3, 1>(); set_lds_attr<1, 1>(); set_lds_attr<5, 2>(); set_lds_attr<3, 2>(); set_lds_attr<1, 2>();
        set_lds_attr<7, 1>(); set_lds_attr<11, 1>(); set_lds_attr<7, 2>(); set_lds_attr<11, 2>(); set_lds_attr<9, 1>(); set_lds_attr<9, 2>();
        set_lds_attr<1, 3>(); set_lds_attr<3, 3>(); set_lds_attr<5, 3>(); set_lds_attr<7, 3>(); set_lds_attr<9, 3>(); set_lds_attr<11, 3>();
        once = true;
    }
}
