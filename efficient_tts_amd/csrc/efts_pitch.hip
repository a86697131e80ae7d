// efts_pitch.hip -- a YIN pitch tracker (de Cheveigne & Kawahara 2002, steps 1 - 5) on the frame grid of the log-mel front-end: efts_yin and
// efts_yin_pcm16.  include/efts_abi.h has the definitions; efficient_tts_amd/pitch.py owns the calls.  fp32, no atomics, every sum in one fixed
// order: an item gives the same bits alone, in any batch position and in any run.
//
// Shape.  One workgroup of YIN_THREADS threads takes G = 4 * (1024 / W) consecutive frames of one item (W = n_fft / 2):
//   * the samples those frames cover are staged ONCE in LDS, reflected at the item's ends and scaled at the load: with hop % 4 == 0 as one
//     span of n_fft + (G - 1) hop samples (neighbouring frames share n_fft - hop of them), otherwise frame by frame, so that every frame
//     starts on a 16-byte boundary either way;
//   * difference function, the direct form: W / 4 threads per frame, thread q owns the four lags 4q + 1 .. 4q + 4 and sweeps j in blocks of
//     four.  Per block it reads x[j .. j + 3] (one 16-byte LDS read, the same address in every lane of the frame: a broadcast) and
//     x[j + 4q + 4 .. j + 4q + 7] (16 bytes, consecutive across lanes); the four samples in front of those are the previous block's read and
//     stay in registers.  Two LDS reads feed 16 subtract + fma pairs, so the loop is bound by the vector ALU, not by LDS;
//   * one wave per frame then turns d into d' in place: a lane owns a contiguous run of lags, sums it, the 64 totals are scanned across the
//     wave, and the lane walks its run again from the total in front of it.  The first lag under the threshold is a per-lane search plus a
//     wave minimum; the walk to the local minimum and the parabola are a handful of broadcast reads.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "efts_internal.h"
#include "efts_stft_frame.h"

namespace efts {

constexpr int YIN_THREADS = 256, YIN_WAVES = YIN_THREADS / 64, YIN_PASSES = 4;

struct yin_geom {
    int n_fft, hop, W, pad, tau_min, tau_max;
    int tpf, fpp, G;            // threads per frame, frames per pass, frames per workgroup
    int fstride, shared_span;   // distance of two frames in LDS (floats); 1: one span of samples, 0: every frame staged on its own
    int xs_floats, ds;          // floats of the sample stage; row stride of d / d'
    float sr, threshold;
};

template <typename T>
__global__ __launch_bounds__(YIN_THREADS) void yin_kernel(const T* __restrict__ audio, long ld, float scale, const int* __restrict__ lengths, yin_geom g,
                                                          int Tout, float* __restrict__ f0, float* __restrict__ aper, float* __restrict__ cmnd) {
    extern __shared__ float4 yin_lds[];
    float* xs = (float*)yin_lds;                           // the staged samples
    float* dv = xs + g.xs_floats;                          // [G][ds]: d(tau), then d'(tau), tau = 0 .. W
    const int b = blockIdx.y, t = threadIdx.x, f_first = blockIdx.x * g.G;
    const int len = max(0, (int)min((long)lengths[b], ld));
    const int frames = len > g.pad ? len / g.hop : 0;      // the front-end's precondition: an item no longer than its padding has no frames
    const int n_rows = min(g.G, Tout - f_first);           // frames of this workgroup that exist in the outputs
    const int n_valid = max(0, min(n_rows, frames - f_first));
    const int cm_ld = g.tau_max + 1;

    // frames at or beyond the item's count: zeros everywhere
    for (int r = n_valid + t / 64; r < n_rows; r += YIN_WAVES) {
        const long row = (long)b * Tout + f_first + r;
        if ((t & 63) == 0) { f0[row] = 0.f; aper[row] = 0.f; }
        if (cmnd)
            for (int k = t & 63; k < cm_ld; k += 64) cmnd[row * cm_ld + k] = 0.f;
    }
    if (n_valid == 0) return;                              // (uniform over the workgroup)

    // stage: sample s of frame f is audio index f hop - pad + s, reflected once at either end (len > pad makes once enough) and clamped
    const T* ab = audio + (long)b * ld;
    const int n_stage = g.shared_span ? g.n_fft + (n_valid - 1) * g.hop : n_valid * g.n_fft;
    for (int p = t; p < n_stage; p += YIN_THREADS) {
        const int f = g.shared_span ? 0 : p / g.n_fft, s = g.shared_span ? p : p - f * g.n_fft;
        long i = (long)(f_first + f) * g.hop - g.pad + s;
        if (i < 0) i = -i;
        if (i >= len) i = 2L * (len - 1) - i;
        i = max(0L, min(i, (long)len - 1));
        xs[p] = pcm_sample(ab, i, scale);
    }
    __syncthreads();

    // d(tau) = sum over j = 0 .. W - 1, ascending and fused, of (x[j] - x[j + tau])^2 for tau = 4q + 1 .. 4q + 4
    const int q = t % g.tpf;
    for (int pass = 0; pass < YIN_PASSES; ++pass) {
        const int fl = pass * g.fpp + t / g.tpf;
        if (fl < n_valid && 4 * q + 1 <= g.tau_max) {
            const float* xf = xs + fl * g.fstride;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            float4 lo = *(const float4*)(xf + 4 * q);
            for (int jb = 0; jb < g.W; jb += 4) {
                const float4 a = *(const float4*)(xf + jb);
                const float4 hi = *(const float4*)(xf + jb + 4 * q + 4);            // last read: floats n_fft - 4 .. n_fft - 1 of the frame
                const float av[4] = {a.x, a.y, a.z, a.w};
                const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float d = av[jj] - w[jj + c + 1];
                        acc[c] = fmaf(d, d, acc[c]);
                    }
                lo = hi;
            }
            float* dr = dv + fl * g.ds + 4 * q + 1;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (4 * q + 1 + c <= g.tau_max) dr[c] = acc[c];
        }
    }
    __syncthreads();

    // one wave per frame: running sum, d', decision.  Every wave makes the same number of rounds, so the barriers are uniform.
    const int lane = t & 63, wave = t >> 6;
    const int ch = (g.tau_max + 63) / 64;                  // lags per lane: lane l owns l ch + 1 .. l ch + ch
    const int k0 = lane * ch + 1, k1 = min(k0 + ch - 1, g.tau_max);
    for (int r0 = 0; r0 < g.G; r0 += YIN_WAVES) {
        const int fl = r0 + wave;
        const bool live = fl < n_valid;
        float* dr = dv + fl * g.ds;
        if (live) {
            float tot = 0.f;
            for (int k = k0; k <= k1; ++k) tot += dr[k];
            const float incl = wave_scan_incl(tot);
            float run = __shfl_up(incl, 1);
            if (lane == 0) run = 0.f;
            for (int k = k0; k <= k1; ++k) {               // a lane rewrites only the lags it alone reads here
                const float d = dr[k];
                run += d;
                dr[k] = run == 0.f ? 1.f : d * (float)k / run;
            }
            if (lane == 0) dr[0] = 1.f;
        }
        __syncthreads();
        if (live) {
            const long row = (long)b * Tout + f_first + fl;
            if (cmnd)
                for (int k = lane; k < cm_ld; k += 64) cmnd[row * cm_ld + k] = dr[k];
            int cand = 0x7fffffff;
            float lowest = __builtin_inff();
            for (int k = max(k0, g.tau_min); k <= min(k1, g.tau_max - 1); ++k) {
                const float v = dr[k];
                lowest = fminf(lowest, v);
                if (v < g.threshold && cand == 0x7fffffff) cand = k;
            }
            int tau = wave_min(cand);
            lowest = wave_min(lowest);
            float pitch = 0.f, ap = lowest;
            if (tau != 0x7fffffff) {                       // (uniform over the wave: the reads below are broadcasts)
                while (tau + 1 <= g.tau_max - 1 && dr[tau + 1] < dr[tau]) ++tau;
                const float s0 = dr[tau - 1], s1 = dr[tau], s2 = dr[tau + 1];
                const float den = (s0 - s1) + (s2 - s1);
                float shift = den == 0.f ? 0.f : 0.5f * (s0 - s2) / den;
                shift = fminf(1.f, fmaxf(-1.f, shift));
                pitch = g.sr / ((float)tau + shift);
                ap = s1;
            }
            if (lane == 0) { f0[row] = pitch; aper[row] = ap; }
        }
    }
}

static int yin_geometry(const char* who, int n_fft, int hop, int sr, float fmin, float fmax, float threshold, yin_geom* g) {
    if (n_fft != 512 && n_fft != 1024 && n_fft != 2048) return efts_fail(EFTS_ESHAPE, "%s: n_fft 512, 1024 or 2048 (got %d)", who, n_fft);
    if (hop < 1 || hop > n_fft || ((n_fft - hop) & 1)) return efts_fail(EFTS_ESHAPE, "%s: hop 1 .. n_fft with n_fft - hop even (got %d)", who, hop);
    if (sr < 1 || !(fmin > 0.f) || !(fmax > fmin) || !isfinite(fmax) || !(threshold > 0.f) || !isfinite(threshold))
        return efts_fail(EFTS_ESHAPE, "%s: sampling_rate >= 1, 0 < fmin < fmax, threshold > 0", who);
    const int W = n_fft / 2;
    const double lo = floor((double)sr / (double)fmax), hi = floor((double)sr / (double)fmin);
    if (lo < 2.0) return efts_fail(EFTS_ESHAPE, "%s: tau_min = floor(sampling_rate / fmax) = %.0f is below 2", who, lo);
    if (hi > (double)W) return efts_fail(EFTS_ESHAPE, "%s: fmin too low: a period of %.0f samples does not fit the %d lags of n_fft %d", who, hi, W, n_fft);
    if (!(lo < hi - 1.0)) return efts_fail(EFTS_ESHAPE, "%s: need tau_min < tau_max - 1 (got %.0f, %.0f)", who, lo, hi);
    g->n_fft = n_fft; g->hop = hop; g->W = W; g->pad = (n_fft - hop) / 2; g->tau_min = (int)lo; g->tau_max = (int)hi;
    g->tpf = W / 4; g->fpp = YIN_THREADS / g->tpf; g->G = g->fpp * YIN_PASSES;
    g->shared_span = hop % 4 == 0;
    g->fstride = g->shared_span ? hop : n_fft;
    g->xs_floats = g->shared_span ? n_fft + (g->G - 1) * hop : g->G * n_fft;      // a multiple of 4 either way: d starts 16-byte aligned
    g->ds = W + 4;
    g->sr = (float)sr; g->threshold = threshold;
    return EFTS_OK;
}

template <typename T>
static int yin_launch(const char* who, const T* audio, int64_t ld, float scale, const int32_t* lengths, float* f0, float* aper, float* cmnd, int B, int Tout,
                      int n_fft, int hop, int sr, float fmin, float fmax, float threshold, void* stream) {
    if (!audio || !lengths || !f0 || !aper) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    yin_geom g;
    const int rc = yin_geometry(who, n_fft, hop, sr, fmin, fmax, threshold, &g);
    if (rc != EFTS_OK) return rc;
    if (B < 1 || B > 65535 || Tout < 1 || ld < 1 || ld > 2147483647LL) return efts_fail(EFTS_ESHAPE, "%s: 1 .. 65535 items, T >= 1, ld 1 .. 2^31 - 1", who);
    const size_t lds = sizeof(float) * ((size_t)g.xs_floats + (size_t)g.G * g.ds);      // at most 50 KiB
    hipLaunchKernelGGL(yin_kernel<T>, dim3((unsigned)((Tout + g.G - 1) / g.G), (unsigned)B), dim3(YIN_THREADS), lds, (hipStream_t)stream, audio, (long)ld, scale,
                       lengths, g, Tout, f0, aper, cmnd);
    return efts_check_launch(who);
}

}  // namespace efts

using namespace efts;

extern "C" int efts_yin(const float* audio, int64_t ld, const int32_t* lengths, float* f0, float* aperiodicity, float* cmnd, int32_t B, int32_t T,
                        int32_t n_fft, int32_t hop, int32_t sampling_rate, float fmin, float fmax, float threshold, void* stream) {
    return yin_launch<float>("efts_yin", audio, ld, 1.f, lengths, f0, aperiodicity, cmnd, B, T, n_fft, hop, sampling_rate, fmin, fmax, threshold, stream);
}

extern "C" int efts_yin_pcm16(const int16_t* audio, int64_t ld, float pcm_scale, const int32_t* lengths, float* f0, float* aperiodicity, float* cmnd,
                              int32_t B, int32_t T, int32_t n_fft, int32_t hop, int32_t sampling_rate, float fmin, float fmax, float threshold,
                              void* stream) {
    return yin_launch<int16_t>("efts_yin_pcm16", audio, ld, pcm_scale, lengths, f0, aperiodicity, cmnd, B, T, n_fft, hop, sampling_rate, fmin, fmax,
                               threshold, stream);
}
