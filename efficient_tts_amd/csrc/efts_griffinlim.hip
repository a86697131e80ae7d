// efts_griffinlim.hip -- Griffin-Lim phase reconstruction (Griffin & Lim 1984; momentum: Perraudin, Balazs & Sondergaard 2013) for
// the analysis configuration of the log-mel front-end: n_fft 1024, hop 256, periodic Hann window, 384 samples of padding on each
// side, frames not centred -- frame t starts at padded sample 256 t, T frames describe the padded signal y_pad of 256 T + 768 samples.
//
//   X [B][T][513] complex --efts_gl_synthesis--> windowed frames wf [B][T][1024] = hann * irfft(X)
//   wf --efts_gl_analysis--> y_pad[p] = (sum of the frames that cover p) / (sum of their hann^2), never stored;
//                            Y = rfft(hann * y_pad[256 t ..]); C = Y + a (Y - Y_prev); X_next = M C / max(|C|, 1e-8); Y_prev = Y
//   wf --efts_gl_overlap_add--> audio = y_pad[start .. start + n_out)
//
// Two launches per iteration.  Both transforms are the front-end's fp32 1024-point FFT in registers and LDS (efts_fft.h), one wave per
// PAIR of neighbouring frames: z = frame_a + i frame_b goes through one complex transform.  The overlap-add is a gather in a fixed
// order (oldest frame first), not an accumulation with atomics: the same input gives the same bits, eager or replayed from a graph.
// The loop is launch- and latency-bound for one utterance (13 MB per iteration at 800 frames), so the grid is B x T / 2 waves, two
// per workgroup, and the Python side replays the whole loop as one graph.
//
// Frames at or beyond frames[b] do not exist for item b: they are neither read nor written, and they add nothing to the sums.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_internal.h"
#include "efts_fft.h"
#include "efts_stft_frame.h"

namespace efts {

using fft::cf;

constexpr int GL_WAVES = 2, GL_N = 1024, GL_HOP = 256, GL_BINS = 513, GL_OVERLAP = GL_N / GL_HOP;

// the pair of frames of this wave; false when there is nothing to do
__device__ __forceinline__ bool gl_pair(const int* __restrict__ frames, int B, int T, int wave, int& b, int& t0, int& nfr, bool& vb) {
    const int PT = (T + 1) >> 1;
    const int pair = blockIdx.x * GL_WAVES + wave;
    if (pair >= B * PT) return false;
    b = pair / PT;
    t0 = 2 * (pair - b * PT);
    nfr = min(max(frames[b], 0), T);
    vb = t0 + 1 < nfr;
    return t0 < nfr;
}

// X0 = M e^(i phi): phi = 0 (mode 0) or uniform in [0, 2 pi) from the counter-based hash of (seed, t * 513 + f) (mode 1) -- the index
// does not hold the item, so an utterance gets the same phases wherever it stands in a batch.  Y_prev = 0.
__global__ __launch_bounds__(256) void gl_init_kernel(const float* __restrict__ mag, cf* __restrict__ X, cf* __restrict__ yprev, long per_item,
                                                      long total, int mode, unsigned seed_h) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float m = mag[i];
    cf x = {m, 0.f};
    if (mode == 1) {
        const unsigned h = hash_u32((unsigned)(i % per_item) ^ seed_h);
        float sn, cs;
        sincospif((float)(h >> 8) * (2.f / 16777216.f), &sn, &cs);
        x = cf{m * cs, m * sn};
    }
    X[i] = x;
    yprev[i] = cf{0.f, 0.f};
}

// spectrum -> windowed frames.  The inverse transform is conj(FFT(conj Z)) / N with Z = X_a + i X_b, Hermitian-extended to 1024 bins;
// the imaginary parts of the DC and Nyquist bins are dropped (what an inverse real FFT does).
__global__ __launch_bounds__(64 * GL_WAVES) void gl_synthesis_kernel(const cf* __restrict__ X, const int* __restrict__ frames,
                                                                     const float* __restrict__ window, float* __restrict__ wf, int B, int T) {
    __shared__ __attribute__((aligned(16))) cf zs[GL_WAVES][16 * fft::PITCH];
    __shared__ cf tw1s[15][64];
    __shared__ cf tw2s[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    fft::fill_twiddles<64 * GL_WAVES>(tw1s, tw2s);
    __syncthreads();                                     // (the only barrier of the block: from here on a wave is on its own)
    int b, t0, nfr; bool vb;
    if (!gl_pair(frames, B, T, wave, b, t0, nfr, vb)) return;
    cf* zw = zs[wave];
    const cf* xa = X + ((long)b * T + t0) * GL_BINS;
    const cf* xb = xa + GL_BINS;
    cf v[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) {
        const int k = 64 * n1 + lane;
        const bool upper = k > GL_N / 2;                 // Z[k] = conj X_a[N - k] + i conj X_b[N - k]
        const int f = upper ? GL_N - k : k;
        cf a = xa[f], c = {0.f, 0.f};
        if (vb) c = xb[f];
        if (f == 0 || f == GL_N / 2) { a.y = 0.f; c.y = 0.f; }
        const float s = upper ? -1.f : 1.f;
        v[n1] = cf{a.x - s * c.y, -(s * a.y + c.x)};     // conj Z
    }
    fft::fft1024(v, zw, tw1s, tw2s, lane);
    float* fa = wf + ((long)b * T + t0) * GL_N;
    float* fb = fa + GL_N;
    constexpr float INV_N = 1.f / GL_N;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = 64 * i + lane;
        const cf w = zw[fft::bin_slot(n)];
        const float h = window[n];
        fa[n] = w.x * INV_N * h;
        if (vb) fb[n] = -w.y * INV_N * h;
    }
}

// windowed frames (or a padded signal) -> spectrum, with the magnitude projection and the momentum term.
//   signal != nullptr: y_pad is read from signal[b][p] instead of being gathered from wf;
//   mag == nullptr   : the plain analysis, xout = Y (yprev is not touched).
__global__ __launch_bounds__(64 * GL_WAVES) void gl_analysis_kernel(const float* __restrict__ wf, const float* __restrict__ signal, long ld_signal,
                                                                    const int* __restrict__ frames, const float* __restrict__ window,
                                                                    const float* __restrict__ mag, cf* __restrict__ yprev, cf* __restrict__ xout,
                                                                    float momentum, int B, int T) {
    __shared__ __attribute__((aligned(16))) cf zs[GL_WAVES][16 * fft::PITCH];
    __shared__ cf tw1s[15][64];
    __shared__ cf tw2s[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    fft::fill_twiddles<64 * GL_WAVES>(tw1s, tw2s);
    __syncthreads();                                     // (the only barrier of the block)
    int b, t0, nfr; bool vb;
    if (!gl_pair(frames, B, T, wave, b, t0, nfr, vb)) return;
    cf* zw = zs[wave];
    float win[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) win[n1] = window[64 * n1 + lane];
    // y_pad[256 t0 + 64 j + lane], j = 0 .. 19: frame b is frame a moved by one hop = 4 values of j
    float sm[20];
    if (signal != nullptr) {
        const float* s = signal + (long)b * ld_signal;
        const int len = GL_HOP * nfr + GL_N - GL_HOP;
#pragma unroll
        for (int j = 0; j < 20; ++j) {
            const int p = GL_HOP * t0 + 64 * j + lane;
            const float x = s[min(p, len - 1)];
            sm[j] = p < len ? x : 0.f;
        }
    } else {
        // sample p lies in hop block c = p / 256 at offset r; frame c - k holds it at n = r + 256 k, k = 0 .. 3.  Every load is issued,
        // from a clamped address, and a frame that does not exist is dropped by a select: fixed order, oldest frame first
        const float* w0 = wf + (long)b * T * GL_N;
#pragma unroll
        for (int j = 0; j < 20; ++j) {
            const int c = t0 + (j >> 2);
            float acc = 0.f, wss = 0.f;
#pragma unroll
            for (int k = GL_OVERLAP - 1; k >= 0; --k) {
                const int t = c - k, n1 = (j & 3) + 4 * k;
                const bool ok = t >= 0 && t < nfr;
                const float x = w0[(long)min(max(t, 0), nfr - 1) * GL_N + 64 * n1 + lane];
                acc += ok ? x : 0.f;
                wss += ok ? win[n1] * win[n1] : 0.f;
            }
            sm[j] = acc / fmaxf(wss, 1e-8f);
        }
    }
    cf v[16];
    st_pair_values(sm, win, vb, v);
    fft::fft1024(v, zw, tw1s, tw2s, lane);
    const long row = ((long)b * T + t0) * GL_BINS;
    auto project = [&](cf y, long idx) {
        if (mag == nullptr) { xout[idx] = y; return; }
        const cf yp = yprev[idx];
        const cf c = y + momentum * (y - yp);
        const float sc = mag[idx] / fmaxf(sqrtf(c.x * c.x + c.y * c.y), 1e-8f);
        xout[idx] = c * sc;
        yprev[idx] = y;
    };
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int f = lane + 64 * i;
        if (f < GL_BINS) {
            const int fn = (GL_N - f) & (GL_N - 1);
            const cf zf = zw[fft::bin_slot(f)], zn = zw[fft::bin_slot(fn)];
            // st_split (efts_stft_frame.h), spelled out: the spectrum itself is stored here, and the zero that X_b's imaginary part is at DC and
            // Nyquist (zf is zn there) keeps the sign it has always had, -0, where st_split's bi is +0 -- no magnitude can tell, a digest can
            project(cf{0.5f * (zf.x + zn.x), 0.5f * (zf.y - zn.y)}, row + f);
            if (vb) project(cf{0.5f * (zf.y + zn.y), -0.5f * (zf.x - zn.x)}, row + GL_BINS + f);
        }
    }
}

// out[b][s] = y_pad[start + s]: the gather of gl_analysis_kernel, one sample per thread; zero outside the item's signal
__global__ __launch_bounds__(256) void gl_overlap_add_kernel(const float* __restrict__ wf, const int* __restrict__ frames, const float* __restrict__ window,
                                                             float* __restrict__ out, long ld_out, int start, int n_out, int T) {
    const int b = blockIdx.y;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_out) return;
    const int nfr = min(max(frames[b], 0), T);
    const int p = start + s;
    float y = 0.f;
    if (nfr > 0 && p < GL_HOP * nfr + GL_N - GL_HOP - start) {
        const float* w0 = wf + (long)b * T * GL_N;
        const int c = p / GL_HOP, r = p - c * GL_HOP;
        float acc = 0.f, wss = 0.f;
#pragma unroll
        for (int k = GL_OVERLAP - 1; k >= 0; --k) {
            const int t = c - k, n = r + GL_HOP * k;
            const bool ok = t >= 0 && t < nfr;
            const float x = w0[(long)min(max(t, 0), nfr - 1) * GL_N + n], h = window[n];
            acc += ok ? x : 0.f;
            wss += ok ? h * h : 0.f;
        }
        y = acc / fmaxf(wss, 1e-8f);
    }
    out[(long)b * ld_out + s] = y;
}

}  // namespace efts

using namespace efts;

static int gl_shape(const char* who, int32_t B, int32_t T) {
    if (B <= 0 || T <= 0) return efts_fail(EFTS_ESHAPE, "%s: bad B / T", who);
    if ((int64_t)B * ((T + 1) / 2) > (int64_t)GL_WAVES * 0x7fffffff || (int64_t)T * GL_HOP + GL_N > 0x7fffffff)
        return efts_fail(EFTS_ESHAPE, "%s: B x T too large for one launch", who);
    return EFTS_OK;
}

static unsigned gl_blocks(int32_t B, int32_t T) { return (unsigned)(((int64_t)B * ((T + 1) / 2) + GL_WAVES - 1) / GL_WAVES); }

extern "C" int efts_gl_init(const float* mag, float* spec, float* spec_prev, int32_t B, int32_t T, int32_t mode, uint32_t seed, void* stream) {
    if (!mag || !spec || !spec_prev) return efts_fail(EFTS_EINVAL, "efts_gl_init: null pointer");
    if (!(mode == 0 || mode == 1)) return efts_fail(EFTS_EINVAL, "efts_gl_init: mode must be 0 (zero phase) or 1 (hashed uniform phase)");
    if (int rc = gl_shape("efts_gl_init", B, T)) return rc;
    const long per_item = (long)T * GL_BINS, total = per_item * B;
    hipLaunchKernelGGL(gl_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mag, (cf*)spec, (cf*)spec_prev,
                       per_item, total, mode, hash_u32(seed));
    return efts_check_launch("efts_gl_init");
}

extern "C" int efts_gl_synthesis(const float* spec, const int32_t* frames, const float* window, float* wframes, int32_t B, int32_t T,
                                 int32_t n_fft, int32_t hop, void* stream) {
    if (!spec || !frames || !window || !wframes) return efts_fail(EFTS_EINVAL, "efts_gl_synthesis: null pointer");
    if (n_fft != GL_N || hop != GL_HOP) return efts_fail(EFTS_ESHAPE, "efts_gl_synthesis: built for n_fft 1024, hop 256");
    if ((uintptr_t)spec & 7) return efts_fail(EFTS_EALIGN, "efts_gl_synthesis: the spectrum must be 8-byte aligned");
    if (int rc = gl_shape("efts_gl_synthesis", B, T)) return rc;
    hipLaunchKernelGGL(gl_synthesis_kernel, dim3(gl_blocks(B, T)), dim3(64 * GL_WAVES), 0, (hipStream_t)stream, (const cf*)spec, frames, window,
                       wframes, B, T);
    return efts_check_launch("efts_gl_synthesis");
}

extern "C" int efts_gl_analysis(const float* wframes, const float* signal, int64_t ld_signal, const int32_t* frames, const float* window,
                                const float* mag, float* spec_prev, float* spec_out, float momentum, int32_t B, int32_t T, int32_t n_fft,
                                int32_t hop, void* stream) {
    if (!frames || !window || !spec_out) return efts_fail(EFTS_EINVAL, "efts_gl_analysis: null pointer");
    if ((wframes == nullptr) == (signal == nullptr)) return efts_fail(EFTS_EINVAL, "efts_gl_analysis: exactly one of wframes and signal");
    if ((mag == nullptr) != (spec_prev == nullptr)) return efts_fail(EFTS_EINVAL, "efts_gl_analysis: mag and spec_prev go together");
    if (!(momentum >= 0.f && momentum < 1.f)) return efts_fail(EFTS_EINVAL, "efts_gl_analysis: momentum must lie in [0, 1)");
    if (n_fft != GL_N || hop != GL_HOP) return efts_fail(EFTS_ESHAPE, "efts_gl_analysis: built for n_fft 1024, hop 256");
    if (((uintptr_t)spec_out | (uintptr_t)spec_prev) & 7) return efts_fail(EFTS_EALIGN, "efts_gl_analysis: the spectra must be 8-byte aligned");
    if (int rc = gl_shape("efts_gl_analysis", B, T)) return rc;
    if (signal && ld_signal < (int64_t)T * GL_HOP + GL_N - GL_HOP)
        return efts_fail(EFTS_ESHAPE, "efts_gl_analysis: a signal row holds 256 T + 768 samples");
    hipLaunchKernelGGL(gl_analysis_kernel, dim3(gl_blocks(B, T)), dim3(64 * GL_WAVES), 0, (hipStream_t)stream, wframes, signal, (long)ld_signal,
                       frames, window, mag, (cf*)spec_prev, (cf*)spec_out, momentum, B, T);
    return efts_check_launch("efts_gl_analysis");
}

extern "C" int efts_gl_overlap_add(const float* wframes, const int32_t* frames, const float* window, float* out, int64_t ld_out, int32_t start,
                                   int32_t n_out, int32_t B, int32_t T, int32_t n_fft, int32_t hop, void* stream) {
    if (!wframes || !frames || !window || !out) return efts_fail(EFTS_EINVAL, "efts_gl_overlap_add: null pointer");
    if (n_fft != GL_N || hop != GL_HOP) return efts_fail(EFTS_ESHAPE, "efts_gl_overlap_add: built for n_fft 1024, hop 256");
    if (int rc = gl_shape("efts_gl_overlap_add", B, T)) return rc;
    if (B > 65535) return efts_fail(EFTS_ESHAPE, "efts_gl_overlap_add: at most 65535 items per launch");
    if (start < 0 || 2 * start > GL_N - GL_HOP || n_out <= 0 || (int64_t)start + n_out > (int64_t)T * GL_HOP + GL_N - GL_HOP - start || ld_out < n_out)
        return efts_fail(EFTS_ESHAPE, "efts_gl_overlap_add: [start, start + n_out) must lie inside the padded signal trimmed by `start` on both sides, ld_out >= n_out");
    hipLaunchKernelGGL(gl_overlap_add_kernel, dim3((unsigned)((n_out + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, wframes, frames,
                       window, out, (long)ld_out, start, n_out, T);
    return efts_check_launch("efts_gl_overlap_add");
}
