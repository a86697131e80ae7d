// efts_stft.hip -- short-time Fourier magnitudes at four FFT sizes and the multi-resolution STFT distance between two signals
// (include/efts_abi.h has the definition; efficient_tts_amd/stft.py is the host side).  Reference: nntts/losses/stft_loss.py
// (stft :12-32, SpectralConvergenceLoss :53, LogSTFTMagnitudeLoss :74), which goes through torch.stft and keeps both spectrograms.
//
//   stft_kernel<N, DIST> : one launch per resolution.  A group of G lanes (16, 32, 64, 64 for N = 256, 512, 1024, 2048: four, two, one,
//                          one group per wave) takes a PAIR of neighbouring frames of one signal through one complex FFT -- frame 2 p
//                          the real part, frame 2 p + 1 the imaginary part, X_a[f] = (Z[f] + conj Z[N - f]) / 2,
//                          X_b[f] = (Z[f] - conj Z[N - f]) / 2i, the front-end's trick -- with the framing (reflection), the int16
//                          scaling and the window at the loads.  DIST = false: the magnitudes go to memory (efts_stft_mag).
//                          DIST = true: the same code runs a second time on the other signal -- a loop of two turns that is NOT unrolled,
//                          so both signals pass through the same instructions and equal samples give equal bits -- and the three sums of
//                          every frame go to the workspace; no spectrogram is written.
//   stft_reduce_kernel   : one workgroup per item adds the frames' sums in float64, in frame order, and writes the cell count.
//
// Pairing x with y in one transform, as the two-real-frames trick would also allow, was not done: the two spectra then come out of
// different roundings and x == y no longer gives a distance of exactly 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_internal.h"
#include "efts_fft.h"
#include "efts_stft_frame.h"

namespace efts {

constexpr int ST_ITER = 8;                     // transforms per group and workgroup: the twiddle tables are filled once per workgroup
constexpr int ST_CHUNK = 1024;                 // frames per step of the reduction

template <int N> struct st_geo;
template <> struct st_geo<256>  { static constexpr int M = 16, P = 1, WAVES = 4; };
template <> struct st_geo<512>  { static constexpr int M = 16, P = 2, WAVES = 4; };
template <> struct st_geo<1024> { static constexpr int M = 16, P = 4, WAVES = 4; };
template <> struct st_geo<2048> { static constexpr int M = 32, P = 2, WAVES = 2; };     // (16.5 KiB of buffer per wave, 15.5 KiB of twiddles)

template <int N> struct st_cfg {
    static constexpr int M = st_geo<N>::M, P = st_geo<N>::P, WAVES = st_geo<N>::WAVES, THREADS = 64 * WAVES;
    static constexpr int G = M * P, TPW = 64 / G;                         // lanes per transform, transforms per wave
    static constexpr int BUF = M * (P == 4 ? fft::PITCH : G + P);         // complex values of one transform's buffer
    static constexpr int NBINS = N / 2 + 1, NB = (NBINS + G - 1) / G;     // bins, bins per lane
    static constexpr int UPB = WAVES * TPW * ST_ITER;                     // frame pairs per workgroup
    static_assert(M * G == N, "N = M x G");
    __device__ static __forceinline__ int slot(int f) {
        if constexpr (P == 4) return fft::bin_slot(f); else return fft::plan<M, P>::slot(f);
    }
    __device__ static __forceinline__ void fill(fft::cf (*tw1s)[G], fft::cf (*tw2s)[M]) {
        if constexpr (P == 4) fft::fill_twiddles<THREADS>(tw1s, tw2s); else fft::fill_twiddles_mp<M, P, THREADS>(tw1s, tw2s);
    }
    __device__ static __forceinline__ void transform(fft::cf (&v)[M], fft::cf* zw, const fft::cf (*tw1s)[G], const fft::cf (*tw2s)[M], int l) {
        if constexpr (P == 4) fft::fft1024(v, zw, tw1s, tw2s, l); else fft::fft_group<M, P>(v, zw, tw1s, tw2s, l);
    }
};

template <int N, bool DIST>
__global__ __launch_bounds__(st_cfg<N>::THREADS) void stft_kernel(const void* __restrict__ x, int x_pcm, long ldx, const void* __restrict__ y, int y_pcm,
                                                                  long ldy, float pcm_scale, const int* __restrict__ lengths, int max_len,
                                                                  const float* __restrict__ window, int H, int W, float* __restrict__ mag,
                                                                  int* __restrict__ frames, float* __restrict__ part, int T_max) {
    using namespace fft;
    typedef st_cfg<N> C;
    constexpr int M = C::M, G = C::G, NB = C::NB, NBINS = C::NBINS;
    __shared__ __attribute__((aligned(16))) cf zs[C::WAVES * C::TPW][C::BUF];
    __shared__ cf tw1s[M - 1][G];
    __shared__ cf tw2s[C::P][M];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / G, l = lane % G;
    const int len = st_len(lengths, b, max_len), T = st_frames(len, N, H);
    const int p0 = blockIdx.x * C::UPB;
    if (!DIST && blockIdx.x == 0 && threadIdx.x == 0) frames[b] = T;
    if (DIST && 2 * p0 >= T) return;                               // (uniform) nothing of this item here; the magnitudes' rows are zeroed below
    C::fill(tw1s, tw2s);
    __syncthreads();
    cf* zw = zs[wave * C::TPW + g];
    float win[M];
    st_window_regs<M, G>(window, W, N, l, win);
    // from here on nothing synchronises more than one group: a group without work just passes
    for (int it = 0; it < ST_ITER; ++it) {
        const int t0 = 2 * (p0 + (it * C::WAVES + wave) * C::TPW + g);
        if (t0 >= (DIST ? T : T_max)) continue;
        const bool va = t0 < T, vb = t0 + 1 < T;
        if (!va) {                                                 // (the magnitudes only) rows at and beyond the item's count are zero
            float* o = mag + ((long)b * T_max + t0) * NBINS;
            for (int f = l; f < NBINS; f += G) { o[f] = 0.f; if (t0 + 1 < T_max) o[NBINS + f] = 0.f; }
            continue;
        }
        float xa[NB], xb[NB];
#pragma unroll 1
        for (int sig = 0; sig < (DIST ? 2 : 1); ++sig) {           // NOT unrolled: one copy of the code serves both signals
            const bool pcm = sig ? y_pcm != 0 : x_pcm != 0;
            const char* base = (const char*)(sig ? y : x);
            const long ld = sig ? ldy : ldx;
            const int s0 = t0 * H - N / 2;
            cf v[M];
            if (pcm) st_load<short, N, M, G>((const short*)base + (long)b * ld, pcm_scale, len, s0, H, vb, l, win, v);
            else     st_load<float, N, M, G>((const float*)base + (long)b * ld, 1.f, len, s0, H, vb, l, win, v);
            C::transform(v, zw, tw1s, tw2s, l);
            float ma[NB], mb[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int f = l + G * i;
                ma[i] = mb[i] = 1.f;
                if (f < NBINS) {
                    float ar, ai, br, bi;
                    st_split(zw[C::slot(f)], zw[C::slot((N - f) & (N - 1))], ar, ai, br, bi);
                    ma[i] = sqrtf(fmaxf(fmaf(ar, ar, ai * ai), 1e-7f));         // stft_loss.py:32
                    mb[i] = sqrtf(fmaxf(fmaf(br, br, bi * bi), 1e-7f));
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the next transform overwrites zw
            if (!DIST) {
                float* o = mag + ((long)b * T_max + t0) * NBINS;
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    const int f = l + G * i;
                    if (f < NBINS) { o[f] = ma[i]; if (t0 + 1 < T_max) o[NBINS + f] = vb ? mb[i] : 0.f; }
                }
            } else if (sig == 0) {
#pragma unroll
                for (int i = 0; i < NB; ++i) { xa[i] = ma[i]; xb[i] = mb[i]; }
            } else {
                // the lane's bins in ascending order, then the G lanes in one tree: v = v + (the v of the lane G / 2 across), .., 1 across
                float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    if (l + G * i < NBINS) {
                        const float da = ma[i] - xa[i], db = mb[i] - xb[i];
                        s[0] = fmaf(da, da, s[0]); s[1] = fmaf(ma[i], ma[i], s[1]); s[2] += fabsf(logf(ma[i]) - logf(xa[i]));      // stft_loss.py:53, :74
                        s[3] = fmaf(db, db, s[3]); s[4] = fmaf(mb[i], mb[i], s[4]); s[5] += fabsf(logf(mb[i]) - logf(xb[i]));
                    }
                }
#pragma unroll
                for (int j = 0; j < 6; ++j)
#pragma unroll
                    for (int o = G / 2; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o);
                if (l == 0) {
                    float* o = part + ((long)b * T_max + t0) * 3;
                    o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
                    if (vb) { o[3] = s[3]; o[4] = s[4]; o[5] = s[5]; }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void stft_reduce_kernel(const float* __restrict__ part, const int* __restrict__ lengths, int max_len, int N, int H, int T_max,
                                                          double* __restrict__ sums, long long* __restrict__ cells) {
    __shared__ float s[3 * ST_CHUNK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = st_frames(st_len(lengths, b, max_len), N, H);
    const float* p = part + (long)b * T_max * 3;
    double acc = 0.0;
    for (int c0 = 0; c0 < T; c0 += ST_CHUNK) {                     // (T is uniform in the workgroup)
        const int n = min(ST_CHUNK, T - c0);
        __syncthreads();
        for (int i = tid; i < 3 * n; i += 256) s[i] = p[3L * c0 + i];
        __syncthreads();
        if (tid < 3)
            for (int i = 0; i < n; ++i) acc += (double)s[3 * i + tid];
    }
    if (tid < 3) sums[3L * b + tid] = acc;
    if (tid == 0) cells[b] = (long long)T * (N / 2 + 1);
}

static const char* st_bad_shape(int32_t B, int32_t max_len, int32_t N, int32_t H, int32_t W) {
    if (N != 256 && N != 512 && N != 1024 && N != 2048) return "the FFT size must be 256, 512, 1024 or 2048";
    if (H < 1 || H > N) return "the hop must lie in 1 .. the FFT size";
    if (W < 2 || W > N) return "the window length must lie in 2 .. the FFT size";
    return efts_audio_bad_shape(B, max_len);
}

template <bool DIST>
static void st_launch(int32_t N, dim3 grid, hipStream_t st, const void* x, int x_pcm, long ldx, const void* y, int y_pcm, long ldy, float pcm_scale,
                      const int* lengths, int max_len, const float* window, int H, int W, float* mag, int* frames, float* part, int T_max) {
#define EFTS_ST(NN) hipLaunchKernelGGL((stft_kernel<NN, DIST>), dim3((grid.x + st_cfg<NN>::UPB - 1) / st_cfg<NN>::UPB, grid.y), dim3(st_cfg<NN>::THREADS), 0, st, \
                                       x, x_pcm, ldx, y, y_pcm, ldy, pcm_scale, lengths, max_len, window, H, W, mag, frames, part, T_max)
    if (N == 256) EFTS_ST(256); else if (N == 512) EFTS_ST(512); else if (N == 1024) EFTS_ST(1024); else EFTS_ST(2048);
#undef EFTS_ST
}

}  // namespace efts

using namespace efts;

extern "C" int efts_stft_mag(const void* audio, int32_t pcm16, float pcm_scale, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window,
                             float* mag, int32_t* frames, int32_t B, int32_t N, int32_t H, int32_t W, void* stream) {
    if (const char* why = st_bad_shape(B, max_len, N, H, W)) return efts_fail(EFTS_EINVAL, "efts_stft_mag: %s", why);
    if (ld < max_len) return efts_fail(EFTS_EINVAL, "efts_stft_mag: the leading dimension is smaller than the longest item");
    if (!audio || !lengths || !window || !mag || !frames) return efts_fail(EFTS_EINVAL, "efts_stft_mag: null pointer");
    if (((uintptr_t)audio % (pcm16 ? 2 : 4)) || ((uintptr_t)lengths & 3) || ((uintptr_t)window & 3) || ((uintptr_t)mag & 3) || ((uintptr_t)frames & 3))
        return efts_fail(EFTS_EINVAL, "efts_stft_mag: a pointer is not aligned to its element");
    const int T_max = 1 + max_len / H;
    st_launch<false>(N, dim3((unsigned)((T_max + 1) / 2), (unsigned)B), (hipStream_t)stream, audio, pcm16, (long)ld, nullptr, 0, 0L, pcm_scale, lengths, max_len,
                     window, H, W, mag, frames, nullptr, T_max);
    return efts_check_launch("efts_stft_mag");
}

extern "C" int64_t efts_stft_dist_workspace_bytes(int32_t B, int32_t max_len, int32_t N, int32_t H) {
    if (st_bad_shape(B, max_len, N, H, 2)) return 0;
    return efts_round16((int64_t)B * (1 + max_len / H) * 3 * (int64_t)sizeof(float));
}

extern "C" int efts_stft_dist(const void* x, int32_t x_pcm16, int64_t ldx, const void* y, int32_t y_pcm16, int64_t ldy, float pcm_scale, const int32_t* lengths,
                              int32_t max_len, const float* window, double* sums, int64_t* cells, void* workspace, int64_t workspace_bytes, int32_t B, int32_t N,
                              int32_t H, int32_t W, void* stream) {
    if (const char* why = st_bad_shape(B, max_len, N, H, W)) return efts_fail(EFTS_EINVAL, "efts_stft_dist: %s", why);
    if (ldx < max_len || ldy < max_len) return efts_fail(EFTS_EINVAL, "efts_stft_dist: a leading dimension is smaller than the longest item");
    if (workspace_bytes < efts_stft_dist_workspace_bytes(B, max_len, N, H))
        return efts_fail(EFTS_EINVAL, "efts_stft_dist: the workspace is smaller than efts_stft_dist_workspace_bytes asks for");
    if (!x || !y || !lengths || !window || !sums || !cells || !workspace) return efts_fail(EFTS_EINVAL, "efts_stft_dist: null pointer");
    if (((uintptr_t)x % (x_pcm16 ? 2 : 4)) || ((uintptr_t)y % (y_pcm16 ? 2 : 4)) || ((uintptr_t)lengths & 3) || ((uintptr_t)window & 3) || ((uintptr_t)sums & 7) ||
        ((uintptr_t)cells & 7) || ((uintptr_t)workspace & 15))
        return efts_fail(EFTS_EINVAL, "efts_stft_dist: a pointer is not aligned to its element (the workspace: to 16 bytes)");
    const int T_max = 1 + max_len / H;
    hipStream_t st = (hipStream_t)stream;
    st_launch<true>(N, dim3((unsigned)((T_max + 1) / 2), (unsigned)B), st, x, x_pcm16, (long)ldx, y, y_pcm16, (long)ldy, pcm_scale, lengths, max_len, window, H, W,
                    nullptr, nullptr, (float*)workspace, T_max);
    hipLaunchKernelGGL(stft_reduce_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)workspace, lengths, max_len, N, H, T_max, sums, (long long*)cells);
    return efts_check_launch("efts_stft_dist");
}
