// efts_limiter.hip -- true-peak metering after ITU-R BS.1770 Annex 2 (4x oversampling) and a look-ahead peak limiter for a padded batch
// (include/efts_abi.h has the definition; efficient_tts_amd/limiter.py is the host side).  Two launches each, no host synchronisation, no
// allocation, no atomics:
//
//   A  tp_meter_kernel / tp_limit_kernel : one workgroup per chunk of EFTS_LIMITER_CHUNK samples of an item, chunk origins at multiples of the
//                           chunk size from the item's start.  The chunk and its halo are staged into LDS once; a thread takes four
//                           consecutive samples at a time, so every LDS read is one aligned 16-byte read and the 75 taps of phases 1..3 run
//                           on 28 registers.  The limiter goes on inside LDS: the needed gain r, the sliding minimum by log-step doubling
//                           (forward windows of 1, 2, 4, .. P samples, then two of them cover 2 H + 1), the box sum in its stated order, the
//                           final min, the product and one 16-byte store per thread.  p, r, m and g never go to memory.  One partial per
//                           chunk goes to the workspace.
//   B  tp_reduce_kernel   : one workgroup per item takes max / min / the integer sum over the item's partials: all independent of order.
//
// The interpolator's table arrives by value in the kernel arguments: the taps are scalar operands of the fma, nothing is loaded for them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "efts_internal.h"

namespace efts {

constexpr int TP_C = EFTS_LIMITER_CHUNK;                   // samples of one workgroup
constexpr int TP_K = 12;                                   // zero crossings per side: taps k = -12 .. 12
constexpr int TP_TAPS = 2 * TP_K + 1;
constexpr int TP_HMAX = EFTS_LIMITER_MAX_HOLD;
constexpr int TP_THREADS = 256, TP_WAVES = TP_THREADS / 64;
constexpr int TP_EMAX = 2 * TP_HMAX;                       // the largest H + S
constexpr int TP_NR = TP_C + 2 * TP_EMAX;                  // the most needed gains of one chunk
constexpr int TP_NX = TP_NR + 2 * TP_K;                    // the most staged samples
constexpr int TP_PAD = 8;                                  // the box sum reads whole groups of four: up to 7 entries behind the last one it uses
static_assert(TP_C % 4 == 0 && TP_K % 4 == 0 && TP_EMAX % 4 == 0, "16-byte LDS reads");

struct tp_taps { float h[3][TP_TAPS]; };                   // phases 1 .. 3; phase 0 is the sample itself

__device__ __forceinline__ float tp_sample(const float* row, int i, float) { return row[i]; }
__device__ __forceinline__ float tp_sample(const short* row, int i, float scale) { return (float)row[i] * scale; }

// xs[j] = x[first + j] for j = 0 .. count - 1, 0 outside [0, len)
template <typename S>
__device__ __forceinline__ void tp_stage(float* xs, const S* row, int first, int count, int len, float scale) {
    for (int j = threadIdx.x; j < count; j += TP_THREADS) {
        const int i = first + j;
        xs[j] = (i >= 0 && i < len) ? tp_sample(row, i, scale) : 0.f;
    }
}

// p of the four samples whose windows begin at xs[u] (u % 4 == 0): sample n is xs[u + 12 + n], its taps xs[u + n .. u + n + 24]
__device__ __forceinline__ void tp_peak4(const float* xs, int u, const tp_taps& t, float p[4]) {
    float w[28];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const float4 v = *(const float4*)(xs + u + 4 * q);
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        float pk = fabsf(w[TP_K + n]);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < TP_TAPS; ++k) acc = fmaf(w[n + k], t.h[q][k], acc);
            pk = fmaxf(pk, fabsf(acc));
        }
        p[n] = pk;
    }
}

__device__ __forceinline__ float tp_block_max(float v, float* sh) {
    v = wave_max(v);
    __syncthreads();                                               // (sh may still be read from the reduction before)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ float tp_block_min(float v, float* sh) {
    v = wave_min(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
}
__device__ __forceinline__ int tp_block_sum(int v, int* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// one partial per chunk: true peak, sample peak, smallest gain, limited samples (as bits)
__device__ __forceinline__ void tp_write_partial(float4* part, float tp, float sp, float gmin, int limited) {
    *part = make_float4(tp, sp, gmin, __int_as_float(limited));
}

// ---- launch A, metering
template <typename S>
__global__ __launch_bounds__(TP_THREADS) void tp_meter_kernel(const S* __restrict__ in, long ld_in, const int* __restrict__ lengths, tp_taps taps,
                                                              float scale, float4* __restrict__ part, int nchunk_max) {
    __shared__ __attribute__((aligned(16))) float xs[TP_C + 2 * TP_K];
    __shared__ float sh[TP_WAVES];
    const int b = blockIdx.y, c0 = blockIdx.x * TP_C;
    const int len = (int)min((long)max(lengths[b], 0), ld_in);
    if (c0 >= len) return;                                         // no sample of the item in this chunk: its partial is never read
    const S* row = in + (long)b * ld_in;
    tp_stage(xs, row, c0 - TP_K, TP_C + 2 * TP_K, len, scale);
    __syncthreads();
    float tp = 0.f, sp = 0.f;
    for (int u = 4 * threadIdx.x; u < TP_C; u += 4 * TP_THREADS) {
        if (c0 + u >= len) break;
        float p[4];
        tp_peak4(xs, u, taps, p);
#pragma unroll
        for (int n = 0; n < 4; ++n)
            if (c0 + u + n < len) {
                tp = fmaxf(tp, p[n]);
                sp = fmaxf(sp, fabsf(xs[u + TP_K + n]));
            }
    }
    tp = tp_block_max(tp, sh);
    sp = tp_block_max(sp, sh);
    if (threadIdx.x == 0) tp_write_partial(part + (long)b * nchunk_max + blockIdx.x, tp, sp, 1.f, 0);
}

// ---- launch A, limiting
template <typename S>
__global__ __launch_bounds__(TP_THREADS) void tp_limit_kernel(const S* __restrict__ in, long ld_in, const int* __restrict__ lengths, tp_taps taps,
                                                              float scale, float ceiling, int H, int Sm, float* __restrict__ out, long ld_out,
                                                              float4* __restrict__ part, int nchunk_max) {
    __shared__ __attribute__((aligned(16))) float xs[TP_NX];
    __shared__ __attribute__((aligned(16))) float ra[TP_NR + TP_PAD];
    __shared__ __attribute__((aligned(16))) float rb[TP_NR + TP_PAD];
    __shared__ __attribute__((aligned(16))) float rr[TP_C];        // r of the chunk's own samples: the doubling overwrites ra
    __shared__ float sh_f[TP_WAVES];
    __shared__ int sh_i[TP_WAVES];
    const int b = blockIdx.y, tid = threadIdx.x, c0 = blockIdx.x * TP_C;
    const int len = (int)min((long)max(lengths[b], 0), ld_in);
    float* orow = out + (long)b * ld_out;
    const int o_end = (int)min((long)TP_C, ld_out - c0);           // outputs of this chunk (ld_out % 4 may be anything)
    const bool vec = (((uintptr_t)orow & 15) == 0);                // c0 % 4 == 0: a group of four inside ld_out is one 16-byte store
    if (c0 >= len) {                                               // behind the item: +0.0, nothing read
        for (int o = 4 * tid; o < o_end; o += 4 * TP_THREADS) {
            if (vec && o + 4 <= o_end) *(float4*)(orow + c0 + o) = make_float4(0.f, 0.f, 0.f, 0.f);
            else for (int n = 0; n < 4 && o + n < o_end; ++n) orow[c0 + o + n] = 0.f;
        }
        return;
    }
    const S* row = in + (long)b * ld_in;
    const int E4 = (H + Sm + 3) & ~3;                              // the halo of r, rounded up to whole groups of four
    const int NR = TP_C + 2 * E4;
    tp_stage(xs, row, c0 - E4 - TP_K, NR + 2 * TP_K, len, scale);
    __syncthreads();
    // p and r over the chunk and E4 samples on either side; r = 1 outside the item
    float tp = 0.f;
    for (int u = 4 * tid; u < NR; u += 4 * TP_THREADS) {
        const int i = c0 - E4 + u;                                 // the first of four samples
        float r[4] = {1.f, 1.f, 1.f, 1.f};
        if (i + 3 >= 0 && i < len) {
            float p[4];
            tp_peak4(xs, u, taps, p);
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (i + n >= 0 && i + n < len) {
                    if (p[n] > ceiling) r[n] = __fdiv_rn(ceiling, p[n]);
                    if (u + n >= E4 && u + n < E4 + TP_C) tp = fmaxf(tp, p[n]);
                }
        }
        *(float4*)(ra + u) = make_float4(r[0], r[1], r[2], r[3]);
        if (u >= E4 && u < E4 + TP_C) *(float4*)(rr + u - E4) = make_float4(r[0], r[1], r[2], r[3]);
    }
    __syncthreads();
    // forward windows: after the pass with step w, cur[u] = min r[u .. u + 2 w - 1] wherever that window lies inside 0 .. NR - 1
    const int L = 2 * H + 1;
    float* cur = ra;
    float* nxt = rb;
    int P = 1;
    for (; 2 * P <= L; P *= 2) {
        for (int u = tid; u < NR; u += TP_THREADS) nxt[u] = u + P < NR ? fminf(cur[u], cur[u + P]) : cur[u];
        __syncthreads();
        float* t = cur; cur = nxt; nxt = t;
    }
    // m over the chunk and Sm samples on either side: m index v is the sample c0 - Sm + v, its window begins at r index v - Sm + E4 - H
    const int NM = TP_C + 2 * Sm;
    for (int v = tid; v < NM + TP_PAD; v += TP_THREADS) {
        const int us = v - Sm + E4 - H;
        nxt[v] = v < NM ? fminf(cur[us], cur[us + L - P]) : 1.f;
    }
    __syncthreads();
    const float* m = nxt;
    // the box sum in ascending order, the mean, g, the product
    const float width = (float)(2 * Sm + 1);
    float gmin = 1.f;
    int limited = 0;
    for (int o = 4 * tid; o < o_end; o += 4 * TP_THREADS) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        const int last = 2 * Sm;                                   // output n adds the window entries n .. n + last of m[o ..]
        for (int e4 = 0; e4 <= last + 3; e4 += 4) {
            const float4 q = *(const float4*)(m + o + e4);
            const float w[4] = {q.x, q.y, q.z, q.w};
            if (e4 >= 4 && e4 + 3 <= last) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int n = 0; n < 4; ++n) a[n] = a[n] + w[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        if (e4 + j >= n && e4 + j <= n + last) a[n] = a[n] + w[j];
            }
        }
        const float4 r4 = *(const float4*)(rr + o);
        const float4 x4 = *(const float4*)(xs + o + E4 + TP_K);
        const float r[4] = {r4.x, r4.y, r4.z, r4.w}, x[4] = {x4.x, x4.y, x4.z, x4.w};
        float y[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const float g = fminf(r[n], __fdiv_rn(a[n], width));
            if (c0 + o + n < len) {
                y[n] = x[n] * g;
                gmin = fminf(gmin, g);
                limited += g < 1.f ? 1 : 0;
            } else {
                y[n] = 0.f;
            }
        }
        if (vec && o + 4 <= o_end) *(float4*)(orow + c0 + o) = make_float4(y[0], y[1], y[2], y[3]);
        else for (int n = 0; n < 4 && o + n < o_end; ++n) orow[c0 + o + n] = y[n];
    }
    tp = tp_block_max(tp, sh_f);
    gmin = tp_block_min(gmin, sh_f);
    limited = tp_block_sum(limited, sh_i);
    if (tid == 0) tp_write_partial(part + (long)b * nchunk_max + blockIdx.x, tp, 0.f, gmin, limited);
}

// ---- launch B
__global__ __launch_bounds__(TP_THREADS) void tp_reduce_kernel(const int* __restrict__ lengths, long ld_in, const float4* __restrict__ part, int nchunk_max,
                                                               float* __restrict__ true_peak, float* __restrict__ sample_peak,
                                                               float* __restrict__ gain_min, int* __restrict__ limited) {
    __shared__ float sh_f[TP_WAVES];
    __shared__ int sh_i[TP_WAVES];
    const int b = blockIdx.x;
    const long len = min((long)max(lengths[b], 0), ld_in);
    const int nchunk = (int)((len + TP_C - 1) / TP_C);
    float tp = 0.f, sp = 0.f, gmin = 1.f;
    int lim = 0;
    for (int c = threadIdx.x; c < nchunk; c += TP_THREADS) {
        const float4 v = part[(long)b * nchunk_max + c];
        tp = fmaxf(tp, v.x);
        sp = fmaxf(sp, v.y);
        gmin = fminf(gmin, v.z);
        lim += __float_as_int(v.w);
    }
    tp = tp_block_max(tp, sh_f);
    sp = tp_block_max(sp, sh_f);
    gmin = tp_block_min(gmin, sh_f);
    lim = tp_block_sum(lim, sh_i);
    if (threadIdx.x != 0) return;
    true_peak[b] = tp;
    if (sample_peak) sample_peak[b] = sp;
    if (gain_min) gain_min[b] = gmin;
    if (limited) limited[b] = lim;
}

static inline int64_t tp_nchunk(int64_t max_len) { return (max_len + TP_C - 1) / TP_C; }
static inline bool tp_ld_ok(int64_t ld) { return ld >= 1 && ld <= 0x7fffffffLL - 4 * 2048; }

static int tp_common_checks(const void* in, size_t elem, int64_t ld_in, const int32_t* lengths, const float* table, float scale, const void* workspace,
                            int32_t B, tp_taps* taps, const char* who) {
    if (B <= 0 || B > 65535) return efts_fail(EFTS_ESHAPE, "%s: 1 .. 65535 items per launch", who);
    if (!tp_ld_ok(ld_in)) return efts_fail(EFTS_ESHAPE, "%s: ld_in must lie in 1 .. 2^31 - 8193", who);
    if (!in || !lengths || !table || !workspace) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (((uintptr_t)in % elem) || ((uintptr_t)lengths & 3) || ((uintptr_t)table & 3) || ((uintptr_t)workspace & 15))
        return efts_fail(EFTS_EINVAL, "%s: misaligned pointer (every array to its element, the workspace to 16 bytes)", who);
    if (!std::isfinite(scale) || !(scale > 0.f)) return efts_fail(EFTS_EINVAL, "%s: pcm_scale must be a positive number", who);
    for (int i = 0; i < 4 * TP_TAPS; ++i)
        if (!std::isfinite(table[i])) return efts_fail(EFTS_EINVAL, "%s: table entry %d is not finite", who, i);
    for (int k = 0; k < TP_TAPS; ++k)
        if (table[k] != (k == TP_K ? 1.f : 0.f)) return efts_fail(EFTS_EINVAL, "%s: phase 0 of the table must be the identity", who);
    for (int q = 0; q < 3; ++q)
        for (int k = 0; k < TP_TAPS; ++k) taps->h[q][k] = table[(q + 1) * TP_TAPS + k];
    return EFTS_OK;
}

template <typename S>
static int true_peak_launch(const S* in, int64_t ld_in, const int32_t* lengths, const float* table, float scale, float* true_peak, float* sample_peak,
                            void* workspace, int32_t B, void* stream, const char* who) {
    tp_taps taps;
    if (const int rc = tp_common_checks(in, sizeof(S), ld_in, lengths, table, scale, workspace, B, &taps, who)) return rc;
    if (!true_peak || !sample_peak) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (((uintptr_t)true_peak & 3) || ((uintptr_t)sample_peak & 3)) return efts_fail(EFTS_EINVAL, "%s: misaligned pointer", who);
    const int nchunk = (int)tp_nchunk(ld_in);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tp_meter_kernel<S>, dim3((unsigned)nchunk, (unsigned)B), dim3(TP_THREADS), 0, st, in, (long)ld_in, lengths, taps, scale,
                       (float4*)workspace, nchunk);
    hipLaunchKernelGGL(tp_reduce_kernel, dim3((unsigned)B), dim3(TP_THREADS), 0, st, lengths, (long)ld_in, (const float4*)workspace, nchunk, true_peak,
                       sample_peak, (float*)nullptr, (int*)nullptr);
    return efts_check_launch(who);
}

template <typename S>
static int peak_limit_launch(const S* in, int64_t ld_in, const int32_t* lengths, const float* table, float scale, float ceiling, int32_t hold,
                             int32_t smooth, float* out, int64_t ld_out, float* gain_min, int32_t* limited, float* true_peak, void* workspace, int32_t B,
                             void* stream, const char* who) {
    tp_taps taps;
    if (!tp_ld_ok(ld_out) || ld_out < ld_in) return efts_fail(EFTS_ESHAPE, "%s: ld_out must lie in ld_in .. 2^31 - 8193", who);
    if (!(smooth >= 1 && smooth <= hold && hold <= TP_HMAX)) return efts_fail(EFTS_ESHAPE, "%s: 1 <= smooth <= hold <= %d", who, TP_HMAX);
    if (const int rc = tp_common_checks(in, sizeof(S), ld_in, lengths, table, scale, workspace, B, &taps, who)) return rc;
    if (!out || !gain_min || !limited || !true_peak) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (((uintptr_t)out & 3) || ((uintptr_t)gain_min & 3) || ((uintptr_t)limited & 3) || ((uintptr_t)true_peak & 3))
        return efts_fail(EFTS_EINVAL, "%s: misaligned pointer", who);
    if (!std::isfinite(ceiling) || !(ceiling > 0.f)) return efts_fail(EFTS_EINVAL, "%s: the ceiling must be a finite number > 0", who);
    const char* in_lo = (const char*)in;
    const char* in_hi = in_lo + ((int64_t)(B - 1) * ld_in + ld_in) * (int64_t)sizeof(S);
    const char* out_lo = (const char*)out;
    const char* out_hi = out_lo + ((int64_t)(B - 1) * ld_out + ld_out) * 4;
    if (in_lo < out_hi && out_lo < in_hi) return efts_fail(EFTS_EINVAL, "%s: out overlaps in (a chunk reads its neighbours' samples)", who);
    const int nchunk = (int)tp_nchunk(ld_in);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tp_limit_kernel<S>, dim3((unsigned)tp_nchunk(ld_out), (unsigned)B), dim3(TP_THREADS), 0, st, in, (long)ld_in, lengths, taps, scale,
                       ceiling, (int)hold, (int)smooth, out, (long)ld_out, (float4*)workspace, nchunk);
    hipLaunchKernelGGL(tp_reduce_kernel, dim3((unsigned)B), dim3(TP_THREADS), 0, st, lengths, (long)ld_in, (const float4*)workspace, nchunk, true_peak,
                       (float*)nullptr, gain_min, limited);
    return efts_check_launch(who);
}

}  // namespace efts

using namespace efts;

extern "C" int64_t efts_limiter_workspace_bytes(int32_t B, int64_t max_len) {
    if (B <= 0 || B > 65535 || !tp_ld_ok(max_len)) return 0;
    return (int64_t)B * tp_nchunk(max_len) * 16;
}

extern "C" int efts_true_peak(const float* in, int64_t ld_in, const int32_t* lengths, const float* table, float* true_peak, float* sample_peak,
                              void* workspace, int32_t B, void* stream) {
    return true_peak_launch<float>(in, ld_in, lengths, table, 1.f, true_peak, sample_peak, workspace, B, stream, "efts_true_peak");
}

extern "C" int efts_true_peak_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, const float* table, float pcm_scale, float* true_peak,
                                    float* sample_peak, void* workspace, int32_t B, void* stream) {
    return true_peak_launch<short>((const short*)in, ld_in, lengths, table, pcm_scale, true_peak, sample_peak, workspace, B, stream, "efts_true_peak_pcm16");
}

extern "C" int efts_peak_limit(const float* in, int64_t ld_in, const int32_t* lengths, const float* table, float ceiling, int32_t hold, int32_t smooth,
                               float* out, int64_t ld_out, float* gain_min, int32_t* limited, float* true_peak, void* workspace, int32_t B, void* stream) {
    return peak_limit_launch<float>(in, ld_in, lengths, table, 1.f, ceiling, hold, smooth, out, ld_out, gain_min, limited, true_peak, workspace, B, stream,
                                    "efts_peak_limit");
}

extern "C" int efts_peak_limit_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, const float* table, float pcm_scale, float ceiling,
                                     int32_t hold, int32_t smooth, float* out, int64_t ld_out, float* gain_min, int32_t* limited, float* true_peak,
                                     void* workspace, int32_t B, void* stream) {
    return peak_limit_launch<short>((const short*)in, ld_in, lengths, table, pcm_scale, ceiling, hold, smooth, out, ld_out, gain_min, limited, true_peak,
                                    workspace, B, stream, "efts_peak_limit_pcm16");
}
