// efts_stft_frame.h -- the paired-frame STFT analysis that the audio kernels share (front-end, STFT distance, mel-cepstra, denoiser, gate, noise
// profile, Griffin-Lim, STOI): the frame count of a centred transform, reflect padding without edge repeat, the int16 scaling and the window at
// the loads, two neighbouring real frames as the real and imaginary part of one complex transform (efts_fft.h), and the split of its result
// into the two spectra.  One definition of each; not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "efts_fft.h"

namespace efts {

// an item's length as the kernels use it, and its frames under torch.stft(center=True): an item of at most N / 2 samples cannot be
// reflect-padded and has none
__device__ __forceinline__ int st_len(const int* __restrict__ lengths, int b, int max_len) { return min(max(lengths[b], 0), max_len); }
__device__ __forceinline__ int st_frames(int len, int N, int H) { return len > N / 2 ? 1 + len / H : 0; }

// index i of the centred, reflect-padded signal (reflection without edge repeat; len > N / 2 keeps one reflection enough)
__device__ __forceinline__ int st_reflect(int s, int len) {
    s = s < 0 ? -s : s;
    s = s >= len ? 2 * (len - 1) - s : s;
    return min(max(s, 0), len - 1);            // (out of range only for a frame past the item's count, whose values are dropped)
}

// sample i of a row: fp32 as it is, int16 PCM times `scale` (rounded once)
template <typename I> __device__ __forceinline__ float pcm_sample(const float* x, I i, float) { return x[i]; }
template <typename I> __device__ __forceinline__ float pcm_sample(const short* x, I i, float scale) { return (float)x[i] * scale; }

// win[n1] = the window at G n1 + l of the frame, a window of W <= N values centred in it
template <int M, int G>
__device__ __forceinline__ void st_window_regs(const float* window, int W, int N, int l, float (&win)[M]) {
    const int off = (N - W) / 2;
#pragma unroll
    for (int n1 = 0; n1 < M; ++n1) {
        const int k = G * n1 + l - off;
        win[n1] = k >= 0 && k < W ? window[k] : 0.f;
    }
}

// v[n1] = (frame a, frame b)[G n1 + l] times the window; frame a begins at sample s0 of the un-padded signal, frame b one hop later
template <typename S, int N, int M, int G>
__device__ __forceinline__ void st_load(const S* __restrict__ a, float scale, int len, int s0, int H, bool vb, int l, const float (&win)[M], fft::cf (&v)[M]) {
    if (s0 >= 0 && s0 + H + N <= len) {        // (uniform in the group) both frames lie inside the item: one base, constant offsets
        const S* p = a + s0 + l;
#pragma unroll
        for (int n1 = 0; n1 < M; ++n1) v[n1] = fft::cf{(float)p[G * n1] * scale * win[n1], (float)p[G * n1 + H] * scale * win[n1]};
    } else {
#pragma unroll
        for (int n1 = 0; n1 < M; ++n1) {
            const int i = s0 + G * n1 + l;
            const float xa = (float)a[st_reflect(i, len)] * scale, xb = (float)a[st_reflect(i + H, len)] * scale;
            v[n1] = fft::cf{xa * win[n1], vb ? xb * win[n1] : 0.f};
        }
    }
}

// N = 1024, hop 256: frame b is frame a moved by 4 values of n1, so 20 loads per lane serve both.  sm[j] is sample s0 + 64 j + lane of the
// pair that begins at sample s0 (frame a: values 0 .. 15, frame b: values 4 .. 19), reflected at the item's ends.  Every load is issued, from
// a clamped address (a predicated load per sample compiled into twenty branches).
template <typename S>
__device__ __forceinline__ void st_load_pair20(const S* __restrict__ x, float scale, int s0, int len, int lane, float (&sm)[20]) {
    if (s0 >= 0 && s0 + 20 * 64 <= len) {      // (wave-uniform) every sample of the pair lies inside the item: one base, constant offsets
        const S* p = x + s0 + lane;
#pragma unroll
        for (int j = 0; j < 20; ++j) sm[j] = pcm_sample(p, 64 * j, scale);
    } else {
#pragma unroll
        for (int j = 0; j < 20; ++j) sm[j] = pcm_sample(x, st_reflect(s0 + 64 * j + lane, len), scale);
    }
}
// ... and the transform's input from them; vb: frame b exists
__device__ __forceinline__ void st_pair_values(const float (&sm)[20], const float (&win)[16], bool vb, fft::cf (&v)[16]) {
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) v[n1] = fft::cf{sm[n1] * win[n1], vb ? sm[n1 + 4] * win[n1] : 0.f};
}

// the two spectra of a pair's transform Z at bin f, zf = Z[f], zn = Z[N - f]: X_a[f] = (Z[f] + conj Z[N - f]) / 2 = ar + i ai,
// X_b[f] = (Z[f] - conj Z[N - f]) / 2i = br + i bi
__device__ __forceinline__ void st_split(fft::cf zf, fft::cf zn, float& ar, float& ai, float& br, float& bi) {
    ar = 0.5f * (zf.x + zn.x), ai = 0.5f * (zf.y - zn.y);
    br = 0.5f * (zf.y + zn.y), bi = 0.5f * (zn.x - zf.x);
}

}  // namespace efts
