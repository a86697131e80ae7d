// efts_trim_energy.h -- the frame energies that the silence trimmer (efts_trim.hip) and the pause shortener (efts_pauses.hip) share: one
// definition (include/efts_abi.h, "Silence trimming and peak normalisation"), one body.  The staging of a span of samples in LDS and launch A.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_internal.h"

namespace efts {

constexpr int TR_THREADS = 256, TR_WAVES = TR_THREADS / 64;
constexpr int TR_SPAN_MAX = 12288;                        // samples of one workgroup of launch A (48 KiB as fp32)
constexpr int TR_F_MAX = 64, TR_R_MAX = 32;               // frames per workgroup, segments per frame
constexpr int TR_PART = TR_F_MAX + TR_R_MAX;              // segment sums of one workgroup (at most F + R - 1)
constexpr int TR_COPY = 4096;                             // outputs of one workgroup of launch C

template <typename S> struct tr_traits;
template <> struct tr_traits<short> {
    typedef unsigned long long energy_t;
    typedef int peak_t;
    static constexpr int V = 8;                           // samples per 16 bytes
    __device__ static __forceinline__ energy_t sq(energy_t acc, short v) { const int x = v; return acc + (energy_t)(unsigned)(x * x); }
    __device__ static __forceinline__ peak_t mag(short v) { const int x = v; return x < 0 ? -x : x; }
};
template <> struct tr_traits<float> {
    typedef float energy_t;
    typedef float peak_t;
    static constexpr int V = 4;
    __device__ static __forceinline__ energy_t sq(energy_t acc, float v) { return fmaf(v, v, acc); }
    __device__ static __forceinline__ peak_t mag(float v) { return fabsf(v); }
};

// Samples s_lo .. s_lo + n_span - 1 of the row into xs[sh + i] (xs 16-byte aligned, room for n_span + V); 0 outside [0, len).
// Only [0, len) of the row is read.  Returns sh.  Ends WITHOUT a barrier.
template <typename S>
__device__ __forceinline__ int tr_stage(S* xs, const S* row, long s_lo, int n_span, int len, int tid) {
    constexpr int V = tr_traits<S>::V;
    const uintptr_t addr = (uintptr_t)row + (intptr_t)s_lo * (intptr_t)sizeof(S);      // of logical sample 0 (an address only: may lie in front of the row)
    const int sh = (int)((addr / sizeof(S)) % V);
    const S* src = (const S*)addr;
    const int i_lo = (int)min((long)n_span, max(0L, -s_lo));
    const int i_hi = max(i_lo, (int)max(0L, min((long)n_span, (long)len - s_lo)));   // src[i_lo .. i_hi) are the item's samples
    const int i_al = min(i_hi, i_lo + (V - (sh + i_lo) % V) % V);                      // first 16-byte boundary inside
    const int nvec = (i_hi - i_al) / V, i_ve = i_al + nvec * V;
    for (int i = tid; i < i_al; i += TR_THREADS) xs[sh + i] = i >= i_lo ? src[i] : (S)0;
    for (int i = i_ve + tid; i < n_span; i += TR_THREADS) xs[sh + i] = i < i_hi ? src[i] : (S)0;
    const uint4* gv = (const uint4*)(src + i_al);
    uint4* lv = (uint4*)(xs + sh + i_al);
    for (int k = tid; k < nvec; k += TR_THREADS) lv[k] = gv[k];
    return sh;
}

// ---- launch A (PEAKS: the chunk peaks as well; the pause shortener needs the energies alone)
template <typename S, bool PEAKS>
__global__ __launch_bounds__(TR_THREADS) void trim_energy_kernel(const S* __restrict__ in, long ld_in, const int* __restrict__ lengths, int W, int H, int F,
                                                                 int seg, int R, typename tr_traits<S>::energy_t* __restrict__ energy,
                                                                 typename tr_traits<S>::peak_t* __restrict__ chunk_peak, int T_max) {
    typedef typename tr_traits<S>::energy_t E;
    typedef typename tr_traits<S>::peak_t P;
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_lds[];
    E* part = (E*)tr_lds;                                          // [TR_PART] segment sums
    S* xs = (S*)(tr_lds + TR_PART * 8);
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = (int)min((long)max(lengths[b], 0), ld_in);
    const int T = (len + H - 1) / H;
    const int f0 = blockIdx.x * F;
    if (f0 >= T) return;                                           // (uniform)
    const int nf = min(F, T - f0), pad = (W - H) / 2;
    const int n_span = (nf - 1) * H + W;
    const int sh = tr_stage(xs, in + (long)b * ld_in, (long)f0 * H - pad, n_span, len, tid);
    __syncthreads();
    const S* x = xs + sh;
    // work items of a wave: the nf + R - 1 segment sums (segment j: `seg` samples from j H), then the nf chunk peaks (chunk k: H samples from pad + k H)
    const int nseg = nf + R - 1;
    for (int w = wave; w < nseg + (PEAKS ? nf : 0); w += TR_WAVES) {
        if (w < nseg) {
            const S* p = x + w * H;
            E acc = 0;
            for (int i = lane; i < seg; i += 64) acc = tr_traits<S>::sq(acc, p[i]);
            acc = wave_sum(acc);
            if (lane == 0) part[w] = acc;
        } else {
            const int k = w - nseg;
            const S* p = x + pad + k * H;
            P m = 0;
            for (int i = lane; i < H; i += 64) { const P v = tr_traits<S>::mag(p[i]); m = v > m ? v : m; }
            m = wave_max_cmp(m);
            if (lane == 0) chunk_peak[(long)b * T_max + f0 + k] = m;
        }
    }
    __syncthreads();
    if (tid < nf) {
        E e = part[tid];
        for (int r = 1; r < R; ++r) e = e + part[tid + r];
        energy[(long)b * T_max + f0 + tid] = e;
    }
}

// The launch of A over [B] rows of ld_in samples: energy [B][T_max], T_max = ceil(ld_in / H) (chunk_peak likewise, unused without PEAKS).
// A frame as W / H hop segments when that divides and a wave has work per segment; else one segment per frame (the frame itself).
template <typename S, bool PEAKS>
static inline void tr_launch_energy(const S* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, typename tr_traits<S>::energy_t* energy,
                                    typename tr_traits<S>::peak_t* chunk_peak, int T_max, int32_t B, hipStream_t st) {
    const bool hops = W % H == 0 && H >= 64;
    const int seg = hops ? H : W, R = hops ? W / H : 1;
    const int F = max(1, min(TR_F_MAX, (TR_SPAN_MAX - W) / H + 1));
    const size_t lds = (size_t)TR_PART * 8 + ((size_t)(F - 1) * H + W + 8) * sizeof(S);
    hipLaunchKernelGGL((trim_energy_kernel<S, PEAKS>), dim3((unsigned)((T_max + F - 1) / F), (unsigned)B), dim3(TR_THREADS), lds, st, in, (long)ld_in, lengths, W,
                       H, F, seg, R, energy, chunk_peak, T_max);
}

}  // namespace efts
