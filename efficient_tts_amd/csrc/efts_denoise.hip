// efts_denoise.hip -- spectral subtraction of a vocoder's stationary "bias" (the tone-and-hiss that a HiFi-GAN generator answers a blank mel
// with): STFT -> m' = max(m - strength * bias, 0) at the frame's own phase -> inverse STFT -> overlap-add, in ONE launch
// (include/efts_abi.h has the definition; efficient_tts_amd/denoise.py is the host side).  N = 1024, hop 256, periodic Hann for analysis and
// synthesis, the centred reflect-padded framing of efts_stft_mag: torch.stft(center=True) -> gain -> torch.istft(length=len).
//
//   denoise_kernel : one WAVE owns a run of DN_RUN = 16 consecutive hops (4096 samples) of one item, four waves (four neighbouring runs) per
//                    workgroup, which share nothing but the twiddle tables.  Output hop c is covered by frames c - 1 .. c + 2, so the run
//                    c0 .. c0 + 15 needs frames c0 - 1 .. c0 + 17.  Frames 2 p and 2 p + 1 of an item always share one complex transform
//                    (frame 2 p the real part), whichever run computes them, so the wave walks the pairs t0 = c0 - 2, c0, .., c0 + 16: ten
//                    pairs, 20 frames for 16 hops (the share that is recomputed by the neighbouring runs: 4 of 20).  Per pair:
//                      load 1280 samples (reflected at the item's ends), window, forward FFT (efts_fft.h: registers + one LDS transpose);
//                      take the two spectra apart by conjugate symmetry, gain per bin, put them together again -- in registers, for all 1024
//                      bins of the Hermitian extension, so no second trip through LDS is needed;
//                      inverse transform as the forward one on the conjugate; synthesis window;
//                      add into a sliding window of 1280 output samples held in REGISTERS (20 per lane, next to 20 sums of window squares):
//                      frame t0 into values 0 .. 15, frame t0 + 1 into 4 .. 19.  After pair t0 the hops t0 - 2 and t0 - 1 are complete: they
//                      are divided by their window sums, stored, and the window slides by eight values.
//                    Every hop therefore receives its frames oldest first, by one wave, without atomics; no spectrum and no frame goes to
//                    memory: the traffic is the audio in (1.25 x through the caches) and the audio out.
//   Items of at most 512 samples, and the zeros behind every item up to ld_out, are written by the same launch before the twiddles are
//   filled (an early exit for runs that hold no sample of their item).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "efts_internal.h"
#include "efts_fft.h"

namespace efts {

using fft::cf;

constexpr int DN_N = 1024, DN_HOP = 256, DN_WAVES = 4;
constexpr int DN_RUN = 16;                               // hops per wave: even, so that a run begins with a pair
constexpr int DN_RUN_SAMPLES = DN_RUN * DN_HOP;
static_assert(DN_RUN % 2 == 0 && DN_RUN >= 4, "a run begins and ends on a pair of frames");

__device__ __forceinline__ int dn_reflect(int s, int len) {
    s = s < 0 ? -s : s;
    s = s >= len ? 2 * (len - 1) - s : s;
    return min(max(s, 0), len - 1);                      // (out of range only for a frame past the item's count, whose values are dropped)
}

__global__ __launch_bounds__(64 * DN_WAVES) void denoise_kernel(const float* __restrict__ audio, long ld, const int* __restrict__ lengths, int max_len,
                                                                const float* __restrict__ window, const float* __restrict__ bias, float strength,
                                                                float* __restrict__ out, long ld_out, int* __restrict__ frames) {
    __shared__ __attribute__((aligned(16))) cf zs[DN_WAVES][16 * fft::PITCH];
    __shared__ cf tw1s[15][64];
    __shared__ cf tw2s[4][16];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = min(max(lengths[b], 0), max_len);
    const int T = len > DN_N / 2 ? 1 + len / DN_HOP : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) frames[b] = T;
    const float* x = audio + (long)b * ld;
    float* o = out + (long)b * ld_out;
    const long g0 = (long)blockIdx.x * (DN_WAVES * DN_RUN_SAMPLES);          // the workgroup's first sample
    if (T == 0 || g0 >= len) {                           // (uniform in the workgroup) a short item passes through; behind an item: zeros
        const long g1 = min(ld_out, g0 + DN_WAVES * DN_RUN_SAMPLES);
        for (long s = g0 + threadIdx.x; s < g1; s += 64 * DN_WAVES) o[s] = s < len ? x[s] : 0.f;
        return;
    }
    fft::fill_twiddles<64 * DN_WAVES>(tw1s, tw2s);
    __syncthreads();                                     // (the only barrier: from here on a wave is on its own)
    const int c0 = (blockIdx.x * DN_WAVES + wave) * DN_RUN;                  // the wave's first hop; g0 < len <= max_len keeps 256 c0 in int
    const long r0 = (long)c0 * DN_HOP, r1 = min(ld_out, r0 + DN_RUN_SAMPLES);
    if (r0 >= len) {                                     // no sample of the item in this run
        for (long s = r0 + lane; s < r1; s += 64) o[s] = 0.f;
        return;
    }
    cf* zw = zs[wave];
    float win[16], bs[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
        const int k = 64 * n1 + lane;
        win[n1] = window[k];
        bs[n1] = strength * bias[k > DN_N / 2 ? DN_N - k : k];
    }
    float acc[20], wss[20];
#pragma unroll
    for (int j = 0; j < 20; ++j) acc[j] = wss[j] = 0.f;
    const int c_last = min(c0 + DN_RUN - 1, (len - 1) / DN_HOP);             // the run's last hop that holds a sample
    constexpr float INV_N = 1.f / DN_N;
    // pair t0 completes hops t0 - 2 and t0 - 1: the walk ends with the pair that completes c_last
    for (int t0 = max(c0 - 2, 0); t0 - 2 <= c_last; t0 += 2) {
        const bool va = t0 < T, vb = t0 + 1 < T;
        if (va) {
            const int s0 = t0 * DN_HOP - DN_N / 2;       // acc[j] is sample s0 + 64 j + lane
            float sm[20];
            if (s0 >= 0 && s0 + DN_N + DN_HOP <= len) {
                const float* p = x + s0 + lane;
#pragma unroll
                for (int j = 0; j < 20; ++j) sm[j] = p[64 * j];
            } else {
#pragma unroll
                for (int j = 0; j < 20; ++j) sm[j] = x[dn_reflect(s0 + 64 * j + lane, len)];
            }
            cf v[16];
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) v[n1] = cf{sm[n1] * win[n1], vb ? sm[n1 + 4] * win[n1] : 0.f};
            fft::fft1024(v, zw, tw1s, tw2s, lane);
            // X_a[k] = (Z[k] + conj Z[N - k]) / 2, X_b[k] = (Z[k] - conj Z[N - k]) / 2i for ALL k (the upper half is the conjugate of the lower
            // one to the bit, so is its gain); Z' = g_a X_a + i g_b X_b; v = conj Z'
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) {
                const int k = 64 * n1 + lane;
                const cf zf = zw[fft::bin_slot(k)], zn = zw[fft::bin_slot((DN_N - k) & (DN_N - 1))];
                const float ar = 0.5f * (zf.x + zn.x), ai = 0.5f * (zf.y - zn.y);
                const float br = 0.5f * (zf.y + zn.y), bi = 0.5f * (zn.x - zf.x);
                const float ma = sqrtf(fmaf(ar, ar, ai * ai)), mb = sqrtf(fmaf(br, br, bi * bi));
                const float da = ma - bs[n1], db = mb - bs[n1];
                const float ga = da > 0.f ? da / ma : 0.f;
                const float gb = (vb && db > 0.f) ? db / mb : 0.f;
                v[n1] = cf{ga * ar - gb * bi, -(ga * ai + gb * br)};
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the next transform overwrites zw
            fft::fft1024(v, zw, tw1s, tw2s, lane);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const cf w = zw[fft::bin_slot(64 * i + lane)];
                const float h = win[i];
                acc[i] += w.x * INV_N * h;
                wss[i] += h * h;
                if (vb) { acc[i + 4] += -w.y * INV_N * h; wss[i + 4] += h * h; }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        // hops t0 - 2 and t0 - 1 are complete: values 0 .. 7
        const long e0 = (long)(t0 - 2) * DN_HOP;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long s = e0 + 64 * j + lane;
            if (s >= r0 && s < r1) o[s] = s < len ? acc[j] / fmaxf(wss[j], 1e-8f) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) { acc[j] = acc[j + 8]; wss[j] = wss[j + 8]; }
#pragma unroll
        for (int j = 12; j < 20; ++j) acc[j] = wss[j] = 0.f;
    }
    // what lies behind the item's last hop in this run
    for (long s = (long)(c_last + 1) * DN_HOP + lane; s < r1; s += 64) o[s] = 0.f;
}

static const char* dn_bad_shape(int32_t B, int32_t max_len) {
    if (B < 1 || B > 65535) return "1 .. 65535 items per launch";
    if (max_len < 1 || max_len > 0x7fffffff - 4 * 2048) return "max_len must lie in 1 .. 2^31 - 8193";
    return nullptr;
}

}  // namespace efts

using namespace efts;

extern "C" int64_t efts_denoise_workspace_bytes(int32_t, int32_t) {
    return 0;                                            // the overlap-add runs in registers: nothing is kept in memory, whatever the arguments
}

extern "C" int efts_denoise(const float* audio, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window, const float* bias,
                            float strength, float* out, int64_t ld_out, int32_t* frames, void* workspace, int64_t workspace_bytes, int32_t B,
                            void* stream) {
    if (const char* why = dn_bad_shape(B, max_len)) return efts_fail(EFTS_EINVAL, "efts_denoise: %s", why);
    if (ld < max_len || ld_out < max_len) return efts_fail(EFTS_EINVAL, "efts_denoise: a leading dimension is smaller than the longest item");
    if (ld_out > 0x7fffffffLL) return efts_fail(EFTS_EINVAL, "efts_denoise: ld_out must stay below 2^31 (every sample of a row is written)");
    if (!(strength >= 0.f) || !std::isfinite(strength)) return efts_fail(EFTS_EINVAL, "efts_denoise: the strength must be a finite number >= 0");
    if (workspace_bytes < efts_denoise_workspace_bytes(B, max_len))
        return efts_fail(EFTS_EINVAL, "efts_denoise: the workspace is smaller than efts_denoise_workspace_bytes asks for");
    if (!audio || !lengths || !window || !bias || !out || !frames) return efts_fail(EFTS_EINVAL, "efts_denoise: null pointer");
    if (((uintptr_t)audio & 3) || ((uintptr_t)lengths & 3) || ((uintptr_t)window & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)out & 3) ||
        ((uintptr_t)frames & 3) || ((uintptr_t)workspace & 15))
        return efts_fail(EFTS_EINVAL, "efts_denoise: a pointer is not aligned to its element (the workspace: to 16 bytes)");
    const uintptr_t a0 = (uintptr_t)audio, a1 = a0 + (uintptr_t)(((int64_t)(B - 1) * ld + max_len) * 4);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((int64_t)B * ld_out * 4);
    if (a0 < o1 && o0 < a1) return efts_fail(EFTS_EINVAL, "efts_denoise: out overlaps audio (the frames of a hop read samples of its neighbours)");
    const int64_t per = (int64_t)DN_WAVES * DN_RUN_SAMPLES;
    hipLaunchKernelGGL(denoise_kernel, dim3((unsigned)((ld_out + per - 1) / per), (unsigned)B), dim3(64 * DN_WAVES), 0, (hipStream_t)stream, audio, (long)ld,
                       lengths, max_len, window, bias, strength, out, (long)ld_out, frames);
    return efts_check_launch("efts_denoise");
}
