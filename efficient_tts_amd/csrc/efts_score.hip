// efts_score.hip -- scoring of synthesised speech against a recording: mel-cepstra of a padded log-mel batch (efts_mel_cepstrum) and the
// cost and length of the dynamic-time-warping path between two padded feature batches (efts_dtw), that path itself (efts_dtw_path: the same
// kernel body, which also records every cell's move and walks them back), and the F0 error along a path (efts_f0_path_error).  include/efts_abi.h has the definitions;
// efficient_tts_amd/score.py builds the DCT table and turns cost / path length into mel-cepstral distortion.  fp32, no atomics, every sum in
// one fixed order, one workgroup per item or pair: an item gives the same bits alone, in any batch and in any run.
//
// efts_dtw.  One workgroup of DTW_THREADS threads per pair walks the cost matrix as an anti-diagonal wavefront and keeps only the wavefront:
//   * rows are dealt in bands of DTW_BAND = DTW_THREADS * DTW_ROWS; inside a band thread t owns rows base + t DTW_ROWS .. + DTW_ROWS - 1, whose
//     x frames stay in registers.  At step s it computes column j = s - t of its rows, top row first, so it needs its own column j - 1
//     (registers), the cell (bottom row of thread t - 1, j) -- which that thread finished in step s - 1 -- and the same row at j - 1, which
//     it read one step earlier (a register).  A band takes Ty + (threads with a row) - 1 steps;
//   * neighbours exchange (A, L) as one 8-byte word through a double-buffered LDS row: step s writes half s & 1 and reads half (s - 1) & 1,
//     so ONE barrier per step orders both the read-after-write and the next overwrite;
//   * the bottom row of a band is the top boundary of the next: the last thread leaves it in an LDS row of Ty words that thread 0 of the
//     next band reads.  In place is safe: word j is read at step j of a band and overwritten at step j + DTW_THREADS - 1;
//   * y goes through an LDS ring of DTW_RING = 2 * DTW_THREADS columns (row stride D' + 1 words: lanes walk it conflict-free), refilled
//     every DTW_THREADS steps with the next DTW_THREADS columns -- the slots they take held columns that the last thread left two steps ago.
// The feature dimension is padded to D' = 16 or 32 with zeros in both operands: (0 - 0)^2 adds exactly nothing to the fused sum.
// Missing predecessors are +inf and the cell in front of (0, 0) is (0, length 0), which turns the start and the two edges into the general
// rule: diagonal first, then (i-1, j), then (i, j-1), each replacing the best so far only when strictly smaller.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "efts_internal.h"

namespace efts {

constexpr int MC_THREADS = 256, MC_ROWS = 32, MC_MAX_MELS = 128, MC_MAX_COEF = 32;
constexpr int DTW_THREADS = 256, DTW_ROWS = 4, DTW_BAND = DTW_THREADS * DTW_ROWS, DTW_RING = 2 * DTW_THREADS, DTW_MAX_DIM = 32;

__global__ __launch_bounds__(MC_THREADS) void mel_cepstrum_kernel(const float* __restrict__ mel, long ld, long item_stride,
                                                                  const int* __restrict__ lengths, int T, const float* __restrict__ table,
                                                                  int n_mels, int n_coef, float* __restrict__ out) {
    __shared__ float tab[MC_MAX_COEF * (MC_MAX_MELS + 1)];
    __shared__ float fr[MC_ROWS * (MC_MAX_MELS + 1)];
    const int b = blockIdx.y, r0 = blockIdx.x * MC_ROWS, tid = threadIdx.x;
    const int st = n_mels | 1;                                         // odd row stride: rows of different lanes fall on different banks
    const int n_rows = min(MC_ROWS, T - r0);                           // rows of this block that exist in the output
    const int n_valid = max(0, min(n_rows, min(lengths[b], T) - r0));  // ... and that belong to the item: the only ones read
    for (int i = tid; i < n_coef * n_mels; i += MC_THREADS) tab[(i / n_mels) * st + i % n_mels] = table[i];
    const float* src = mel + (long)b * item_stride + (long)r0 * ld;
    for (int i = tid; i < n_valid * n_mels; i += MC_THREADS) fr[(i / n_mels) * st + i % n_mels] = src[(long)(i / n_mels) * ld + i % n_mels];
    __syncthreads();
    float* dst = out + ((long)b * T + r0) * n_coef;
    for (int i = tid; i < n_rows * n_coef; i += MC_THREADS) {
        const int r = i / n_coef, k = i - r * n_coef;
        float v = 0.f;
        if (r < n_valid)
            for (int n = 0; n < n_mels; ++n) v = fmaf(tab[k * st + n], fr[r * st + n], v);
        dst[i] = v;
    }
}

template <int DP, bool PATH>
__global__ __launch_bounds__(DTW_THREADS) void dtw_kernel(const float* __restrict__ x, long ldx, long x_item_stride, const int* __restrict__ x_lengths,
                                                          int Tx, const float* __restrict__ y, long ldy, long y_item_stride,
                                                          const int* __restrict__ y_lengths, int Ty, int D, float* __restrict__ cost,
                                                          int* __restrict__ path_len, unsigned char* __restrict__ moves, long moves_item_stride,
                                                          int2* __restrict__ path) {
    extern __shared__ float2 dtw_lds[];
    __shared__ int bt[3];                                  // PATH: the back-trace's cell (i, j) and its position on the path
    constexpr int YS = DP + 1;
    float2* ex = dtw_lds;                                  // [2][DTW_THREADS]: (A, L) of every thread's bottom row, by step parity
    float2* edge = ex + 2 * DTW_THREADS;                   // [Ty]: (A, L) of the row above the band
    float* ys = (float*)(edge + Ty);                       // [DTW_RING][YS]: columns of y
    const int b = blockIdx.x, t = threadIdx.x;
    const int tx = min(x_lengths[b], Tx), ty = min(y_lengths[b], Ty);
    if (tx < 1 || ty < 1) {                                // (uniform over the workgroup: nothing of the item is read)
        if (t == 0) { cost[b] = __builtin_nanf(""); path_len[b] = 0; }
        return;
    }
    const float* xb = x + (long)b * x_item_stride;
    const float* yb = y + (long)b * y_item_stride;
    const float INF = __builtin_inff();
    const long band_steps = (long)Ty + DTW_THREADS - 1;    // PATH: steps reserved per band in `moves`
    unsigned char* mv = PATH ? moves + (long)b * moves_item_stride : nullptr;
    for (int base = 0; base < tx; base += DTW_BAND) {
        const int nt = (min(DTW_BAND, tx - base) + DTW_ROWS - 1) / DTW_ROWS;       // threads of this band that own a row
        const int i0 = base + t * DTW_ROWS;
        float xr[DTW_ROWS][DP];
#pragma unroll
        for (int r = 0; r < DTW_ROWS; ++r)
#pragma unroll
            for (int k = 0; k < DP; ++k) xr[r][k] = (i0 + r < tx && k < D) ? xb[(long)(i0 + r) * ldx + k] : 0.f;
        float leftA[DTW_ROWS];
        int leftL[DTW_ROWS];
#pragma unroll
        for (int r = 0; r < DTW_ROWS; ++r) { leftA[r] = INF; leftL[r] = 0; }
        float cornerA = i0 == 0 ? 0.f : INF;               // the cell above-left of the thread's top row: column j - 1 of the row above
        int cornerL = 0;
        const int steps = ty + nt - 1;
        for (int s = 0; s < steps; ++s) {
            if ((s & (DTW_THREADS - 1)) == 0) {            // columns s .. s + DTW_THREADS - 1 enter the ring (zeros behind the item's end)
                for (int i = t; i < DTW_THREADS * DP; i += DTW_THREADS) {
                    const int j = s + i / DP, k = i % DP;
                    ys[(j & (DTW_RING - 1)) * YS + k] = (j < ty && k < D) ? yb[(long)j * ldy + k] : 0.f;
                }
                __syncthreads();
            }
            const int j = s - t;
            if (t < nt && j >= 0 && j < ty) {
                const float2 top = t > 0 ? ex[((s - 1) & 1) * DTW_THREADS + t - 1] : base > 0 ? edge[j] : make_float2(INF, 0.f);
                float yv[DP];
#pragma unroll
                for (int k = 0; k < DP; ++k) yv[k] = ys[(j & (DTW_RING - 1)) * YS + k];
                float dgA = cornerA, upA = top.x;
                int dgL = cornerL, upL = __float_as_int(top.y);
                unsigned won = 0;                          // PATH: the winning predecessor of each row, 2 bits: 0 diagonal, 1 (i-1, j), 2 (i, j-1)
#pragma unroll
                for (int r = 0; r < DTW_ROWS; ++r) {
                    float acc = 0.f;
#pragma unroll
                    for (int k = 0; k < DP; ++k) {
                        const float d = xr[r][k] - yv[k];
                        acc = fmaf(d, d, acc);
                    }
                    float best = dgA;
                    int len = dgL;
                    unsigned code = 0;
                    if (upA < best) { best = upA; len = upL; code = 1; }
                    if (leftA[r] < best) { best = leftA[r]; len = leftL[r]; code = 2; }
                    if constexpr (PATH) won |= code << (2 * r);
                    dgA = leftA[r];                        // this row's column j - 1 is the next row's diagonal
                    dgL = leftL[r];
                    upA = leftA[r] = sqrtf(acc) + best;
                    upL = leftL[r] = len + 1;
                }
                cornerA = top.x;
                cornerL = __float_as_int(top.y);
                const float2 bottom = make_float2(leftA[DTW_ROWS - 1], __int_as_float(leftL[DTW_ROWS - 1]));
                ex[(s & 1) * DTW_THREADS + t] = bottom;
                if (t == DTW_THREADS - 1) edge[j] = bottom;
                if constexpr (PATH) mv[((long)(base / DTW_BAND) * band_steps + s) * DTW_THREADS + t] = (unsigned char)won;      // one step: 256 contiguous bytes
                if (j == ty - 1) {
#pragma unroll
                    for (int r = 0; r < DTW_ROWS; ++r)
                        if (i0 + r == tx - 1) {
                            cost[b] = leftA[r];
                            path_len[b] = leftL[r];
                            if constexpr (PATH) { bt[0] = tx - 1; bt[1] = ty - 1; bt[2] = leftL[r] - 1; }
                        }
                }
            }
            __syncthreads();
        }
    }
    if constexpr (PATH) {
        // Back-trace, last cell first, written at its final position: path[k] for k = path_len - 1 .. 0.  The move of cell (i, j) is byte
        // (band, step j + thread, thread) of `moves`; going back, the step never grows inside a band, so the bytes are staged through LDS
        // as windows of BT_STEPS whole steps (one contiguous copy, the y ring's space) that lane 0 walks until it leaves the window or the
        // band.  The barrier that ended the last step ordered this workgroup's stores to `moves` before these loads.
        constexpr int BT_STEPS = 64;
        static_assert(BT_STEPS * DTW_THREADS <= (int)sizeof(float) * DTW_RING * YS, "the window lives in the y ring");
        unsigned char* win = (unsigned char*)ys;
        int2* pb = path + (long)b * ((long)Tx + Ty - 1);
        for (;;) {
            const int i = bt[0], j = bt[1];
            if (i < 0) break;                              // (uniform over the workgroup)
            const int band = i / DTW_BAND, s_hi = j + (i % DTW_BAND) / DTW_ROWS, s_lo = max(0, s_hi - (BT_STEPS - 1));
            const uint4* src = (const uint4*)(mv + ((long)band * band_steps + s_lo) * DTW_THREADS);
            for (int w = t; w < (s_hi - s_lo + 1) * (DTW_THREADS / 16); w += DTW_THREADS) ((uint4*)win)[w] = src[w];
            __syncthreads();
            if (t == 0) {
                int ci = i, cj = j, k = bt[2];
                for (;;) {
                    if (k < 0 || ci < 0 || cj < 0) { ci = -1; break; }         // cannot happen with the moves of the forward pass: never write outside `path`
                    pb[k] = make_int2(ci, cj);
                    if (ci == 0 && cj == 0) { ci = -1; break; }
                    const int ct = (ci % DTW_BAND) / DTW_ROWS, s = cj + ct;
                    if (ci / DTW_BAND != band || s < s_lo) break;              // the next window starts at this cell (it is written once more, the same)
                    const unsigned code = (win[(s - s_lo) * DTW_THREADS + ct] >> (2 * (ci % DTW_ROWS))) & 3u;
                    ci -= code != 2u;
                    cj -= code != 1u;
                    --k;
                }
                bt[0] = ci; bt[1] = cj; bt[2] = k;
            }
            __syncthreads();
        }
    }
}

// One workgroup per item.  Thread t takes path cells t, t + F0_THREADS, ...; the per-thread sums are added pairwise through LDS in one fixed tree.
constexpr int F0_THREADS = 256;
__global__ __launch_bounds__(F0_THREADS) void f0_path_error_kernel(const float* __restrict__ f0_a, long lda, int Ta, const float* __restrict__ f0_b, long ldb,
                                                                   int Tb, const int2* __restrict__ path, long path_item_stride,
                                                                   const int* __restrict__ path_len, float* __restrict__ rmse_cents,
                                                                   float* __restrict__ vuv_error, int* __restrict__ voiced_pairs) {
    __shared__ float sq[F0_THREADS];
    __shared__ int nv[F0_THREADS], nd[F0_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = max(0, (int)min((long)path_len[b], path_item_stride));
    const int2* pb = path + (long)b * path_item_stride;
    float acc = 0.f;
    int both = 0, differ = 0;
    for (int k = t; k < n; k += F0_THREADS) {
        const int2 c = pb[k];
        const float a = c.x >= 0 && c.x < Ta ? f0_a[(long)b * lda + c.x] : 0.f;      // a cell outside the contours counts as unvoiced on that side
        const float v = c.y >= 0 && c.y < Tb ? f0_b[(long)b * ldb + c.y] : 0.f;
        const bool va = a > 0.f, vb = v > 0.f;
        if (va && vb) {
            const float cents = 1200.f * log2f(a / v);
            acc = fmaf(cents, cents, acc);
            ++both;
        }
        differ += va != vb;
    }
    sq[t] = acc; nv[t] = both; nd[t] = differ;
    __syncthreads();
    for (int o = F0_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) { sq[t] += sq[t + o]; nv[t] += nv[t + o]; nd[t] += nd[t + o]; }
        __syncthreads();
    }
    if (t == 0) {
        const float nan = __builtin_nanf("");
        voiced_pairs[b] = nv[0];
        rmse_cents[b] = nv[0] > 0 ? sqrtf(sq[0] / (float)nv[0]) : nan;
        vuv_error[b] = n > 0 ? (float)nd[0] / (float)n : nan;
    }
}

template <int DP, bool PATH>
static int dtw_launch(size_t lds, int B, hipStream_t stream, const float* x, long ldx, long sx, const int* xl, int Tx, const float* y, long ldy,
                      long sy, const int* yl, int Ty, int D, float* cost, int* path_len, unsigned char* moves = nullptr, long moves_stride = 0,
                      int2* path = nullptr) {
    const char* who = PATH ? "efts_dtw_path" : "efts_dtw";
    // more than 64 KiB of dynamic LDS is an opt-in per device: asked for on every call that needs it (a host-side attribute, no launch)
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)dtw_kernel<DP, PATH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return efts_fail(EFTS_ELAUNCH, "%s: %zu bytes of LDS refused: %s", who, lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL((dtw_kernel<DP, PATH>), dim3((unsigned)B), dim3(DTW_THREADS), lds, stream, x, ldx, sx, xl, Tx, y, ldy, sy, yl, Ty, D, cost, path_len,
                       moves, moves_stride, path);
    return efts_check_launch(who);
}

}  // namespace efts

using namespace efts;

extern "C" int efts_mel_cepstrum(const float* mel, int64_t ld, int64_t item_stride, const int32_t* lengths, const float* table, float* out, int32_t B,
                                 int32_t T, int32_t n_mels, int32_t n_coef, void* stream) {
    if (!mel || !lengths || !table || !out) return efts_fail(EFTS_EINVAL, "efts_mel_cepstrum: null pointer");
    if (n_mels < 1 || n_mels > MC_MAX_MELS || n_coef < 1 || n_coef > MC_MAX_COEF)
        return efts_fail(EFTS_ESHAPE, "efts_mel_cepstrum: n_mels 1 .. %d, n_coef 1 .. %d", MC_MAX_MELS, MC_MAX_COEF);
    if (B < 1 || B > 65535 || T < 1 || ld < n_mels || item_stride < 0)
        return efts_fail(EFTS_ESHAPE, "efts_mel_cepstrum: 1 .. 65535 items, T >= 1, ld >= n_mels, item_stride >= 0");
    hipLaunchKernelGGL(mel_cepstrum_kernel, dim3((unsigned)((T + MC_ROWS - 1) / MC_ROWS), (unsigned)B), dim3(MC_THREADS), 0, (hipStream_t)stream, mel,
                       (long)ld, (long)item_stride, lengths, T, table, n_mels, n_coef, out);
    return efts_check_launch("efts_mel_cepstrum");
}

extern "C" int efts_dtw(const float* x, int64_t ldx, int64_t x_item_stride, const int32_t* x_lengths, int32_t Tx, const float* y, int64_t ldy,
                        int64_t y_item_stride, const int32_t* y_lengths, int32_t Ty, int32_t D, float* cost, int32_t* path_len, int32_t B,
                        void* stream) {
    if (!x || !x_lengths || !y || !y_lengths || !cost || !path_len) return efts_fail(EFTS_EINVAL, "efts_dtw: null pointer");
    if (D < 1 || D > DTW_MAX_DIM) return efts_fail(EFTS_ESHAPE, "efts_dtw: D 1 .. %d", DTW_MAX_DIM);
    if (Tx < 1 || Tx > EFTS_DTW_MAX_FRAMES || Ty < 1 || Ty > EFTS_DTW_MAX_FRAMES)
        return efts_fail(EFTS_ESHAPE, "efts_dtw: Tx and Ty 1 .. %d frames (got %d, %d)", EFTS_DTW_MAX_FRAMES, Tx, Ty);
    if (B < 1 || B > 65535 || ldx < D || ldy < D || x_item_stride < 0 || y_item_stride < 0)
        return efts_fail(EFTS_ESHAPE, "efts_dtw: 1 .. 65535 pairs, row strides >= D, item strides >= 0");
    const int DP = D <= 16 ? 16 : 32;
    const size_t lds = sizeof(float2) * (2 * DTW_THREADS + (size_t)Ty) + sizeof(float) * DTW_RING * (DP + 1);
    if (DP == 16)
        return dtw_launch<16, false>(lds, B, (hipStream_t)stream, x, (long)ldx, (long)x_item_stride, x_lengths, Tx, y, (long)ldy, (long)y_item_stride, y_lengths,
                              Ty, D, cost, path_len);
    return dtw_launch<32, false>(lds, B, (hipStream_t)stream, x, (long)ldx, (long)x_item_stride, x_lengths, Tx, y, (long)ldy, (long)y_item_stride, y_lengths, Ty,
                          D, cost, path_len);
}

extern "C" int64_t efts_dtw_path_workspace_bytes(int32_t Tx, int32_t Ty) {
    if (Tx < 1 || Tx > EFTS_DTW_MAX_FRAMES || Ty < 1 || Ty > EFTS_DTW_MAX_FRAMES) return 0;
    return (int64_t)((Tx + DTW_BAND - 1) / DTW_BAND) * ((int64_t)Ty + DTW_THREADS - 1) * DTW_THREADS;      // (band, step, thread): one byte each
}

extern "C" int efts_dtw_path(const float* x, int64_t ldx, int64_t x_item_stride, const int32_t* x_lengths, int32_t Tx, const float* y, int64_t ldy,
                             int64_t y_item_stride, const int32_t* y_lengths, int32_t Ty, int32_t D, float* cost, int32_t* path_len, int32_t* path,
                             void* workspace, int64_t workspace_bytes, int32_t B, void* stream) {
    if (!x || !x_lengths || !y || !y_lengths || !cost || !path_len || !path || !workspace) return efts_fail(EFTS_EINVAL, "efts_dtw_path: null pointer");
    if (D < 1 || D > DTW_MAX_DIM) return efts_fail(EFTS_ESHAPE, "efts_dtw_path: D 1 .. %d", DTW_MAX_DIM);
    if (Tx < 1 || Tx > EFTS_DTW_MAX_FRAMES || Ty < 1 || Ty > EFTS_DTW_MAX_FRAMES)
        return efts_fail(EFTS_ESHAPE, "efts_dtw_path: Tx and Ty 1 .. %d frames (got %d, %d)", EFTS_DTW_MAX_FRAMES, Tx, Ty);
    if (B < 1 || B > 65535 || ldx < D || ldy < D || x_item_stride < 0 || y_item_stride < 0)
        return efts_fail(EFTS_ESHAPE, "efts_dtw_path: 1 .. 65535 pairs, row strides >= D, item strides >= 0");
    const int64_t per_pair = efts_dtw_path_workspace_bytes(Tx, Ty);
    if (workspace_bytes < per_pair * B)
        return efts_fail(EFTS_ESHAPE, "efts_dtw_path: the workspace holds %lld bytes, %d pairs of %d x %d frames need %lld", (long long)workspace_bytes, B, Tx, Ty,
                         (long long)(per_pair * B));
    if (((uintptr_t)workspace & 15) || ((uintptr_t)path & 7)) return efts_fail(EFTS_EALIGN, "efts_dtw_path: workspace 16-byte, path 8-byte aligned");
    const int DP = D <= 16 ? 16 : 32;
    const size_t lds = sizeof(float2) * (2 * DTW_THREADS + (size_t)Ty) + sizeof(float) * DTW_RING * (DP + 1);
    if (DP == 16)
        return dtw_launch<16, true>(lds, B, (hipStream_t)stream, x, (long)ldx, (long)x_item_stride, x_lengths, Tx, y, (long)ldy, (long)y_item_stride,
                                    y_lengths, Ty, D, cost, path_len, (unsigned char*)workspace, (long)per_pair, (int2*)path);
    return dtw_launch<32, true>(lds, B, (hipStream_t)stream, x, (long)ldx, (long)x_item_stride, x_lengths, Tx, y, (long)ldy, (long)y_item_stride, y_lengths,
                                Ty, D, cost, path_len, (unsigned char*)workspace, (long)per_pair, (int2*)path);
}

extern "C" int efts_f0_path_error(const float* f0_a, int64_t lda, int32_t Ta, const float* f0_b, int64_t ldb, int32_t Tb, const int32_t* path,
                                  int64_t path_item_stride, const int32_t* path_len, float* f0_rmse_cents, float* vuv_error, int32_t* voiced_pairs,
                                  int32_t B, void* stream) {
    if (!f0_a || !f0_b || !path || !path_len || !f0_rmse_cents || !vuv_error || !voiced_pairs) return efts_fail(EFTS_EINVAL, "efts_f0_path_error: null pointer");
    if (B < 1 || Ta < 1 || Tb < 1 || lda < Ta || ldb < Tb || path_item_stride < 1 || path_item_stride > 2147483647LL)
        return efts_fail(EFTS_ESHAPE, "efts_f0_path_error: B, Ta, Tb >= 1, row strides >= Ta, Tb, path_item_stride 1 .. 2^31 - 1 cells");
    if ((uintptr_t)path & 7) return efts_fail(EFTS_EALIGN, "efts_f0_path_error: path 8-byte aligned");
    hipLaunchKernelGGL(f0_path_error_kernel, dim3((unsigned)B), dim3(F0_THREADS), 0, (hipStream_t)stream, f0_a, (long)lda, Ta, f0_b, (long)ldb, Tb,
                       (const int2*)path, (long)path_item_stride, path_len, f0_rmse_cents, vuv_error, voiced_pairs);
    return efts_check_launch("efts_f0_path_error");
}
