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
//
// The same body, instantiated a second time, is the spectral gate for corpora (`efts_spectral_gate`): a profile row per item instead of one
// bias, a floor under the gain, int16 PCM scaled at the load, and a per-item bypass that takes the copy path of the short items.  The
// instantiation of `efts_denoise` keeps its arithmetic, instruction for instruction, and two waves per SIMD (DESIGN has the register counts).
//
// `efts_noise_profile` measures such a profile from an item's own quiet frames, in four launches on one stream, no atomics, nothing read back:
//   np_energy_kernel : one wave per frame: e[t] = sum of (w x)^2 in float64.
//   np_select_kernel : one workgroup per item, on the energies alone: e_max, the noise frames' flags (e[t] r < e_max), their count K per item
//                      and per run of NP_RUN = 16 frames, and the level of the floor.
//   np_accum_kernel  : one wave per run.  A workgroup none of whose four runs holds a noise frame leaves before the twiddles are filled.  The
//                      wave walks the run's pairs of frames, transforms those with a noise frame in them exactly as denoise_kernel does,
//                      and adds the noise frames' magnitudes in float64 REGISTERS (bins 64 j + lane, j = 0 .. 7, and bin 512): 9 per lane.
//                      One partial row [513] per run with a noise frame goes to the workspace.
//   np_reduce_kernel : one workgroup per item: the runs' rows in ascending order, divided by K, rounded once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "efts_internal.h"
#include "efts_fft.h"
#include "efts_stft_frame.h"

namespace efts {

using fft::cf;

constexpr int DN_N = 1024, DN_HOP = 256, DN_WAVES = 4;
constexpr int DN_RUN = 16;                               // hops per wave: even, so that a run begins with a pair
constexpr int DN_RUN_SAMPLES = DN_RUN * DN_HOP;
static_assert(DN_RUN % 2 == 0 && DN_RUN >= 4, "a run begins and ends on a pair of frames");

// the magnitude that every gain and every profile is taken from (the pair loader and the split of the two spectra: efts_stft_frame.h)
__device__ __forceinline__ float dn_mag(float re, float im) { return sqrtf(fmaf(re, re, im * im)); }

// GATE = false, S = float: efts_denoise (ld_bias, floor, pcm_scale and bypass are not looked at).  GATE = true: efts_spectral_gate.
template <typename S, bool GATE>
__global__ __launch_bounds__(64 * DN_WAVES) void denoise_kernel(const S* __restrict__ audio, long ld, const int* __restrict__ lengths, int max_len,
                                                                const float* __restrict__ window, const float* __restrict__ bias, long ld_bias,
                                                                float strength, float floor, float pcm_scale, const int* __restrict__ bypass,
                                                                float* __restrict__ out, long ld_out, int* __restrict__ frames) {
    __shared__ __attribute__((aligned(16))) cf zs[DN_WAVES][16 * fft::PITCH];
    __shared__ cf tw1s[15][64];
    __shared__ cf tw2s[4][16];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = st_len(lengths, b, max_len), T = st_frames(len, DN_N, DN_HOP);
    if (blockIdx.x == 0 && threadIdx.x == 0) frames[b] = T;
    const S* x = audio + (long)b * ld;
    float* o = out + (long)b * ld_out;
    const long g0 = (long)blockIdx.x * (DN_WAVES * DN_RUN_SAMPLES);          // the workgroup's first sample
    bool pass = T == 0;
    if (GATE) {
        if (bypass != nullptr && bypass[b] != 0) pass = true;
        bias += (long)b * ld_bias;
    }
    if (pass || g0 >= len) {                             // (uniform in the workgroup) a short or bypassed item passes through; behind an item: zeros
        const long g1 = min(ld_out, g0 + DN_WAVES * DN_RUN_SAMPLES);
        for (long s = g0 + threadIdx.x; s < g1; s += 64 * DN_WAVES) o[s] = s < len ? pcm_sample(x, s, pcm_scale) : 0.f;
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
            st_load_pair20(x, pcm_scale, s0, len, lane, sm);
            cf v[16];
            st_pair_values(sm, win, vb, v);
            fft::fft1024(v, zw, tw1s, tw2s, lane);
            // X_a[k] = (Z[k] + conj Z[N - k]) / 2, X_b[k] = (Z[k] - conj Z[N - k]) / 2i for ALL k (the upper half is the conjugate of the lower
            // one to the bit, so is its gain); Z' = g_a X_a + i g_b X_b; v = conj Z'
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1) {
                const int k = 64 * n1 + lane;
                const cf zf = zw[fft::bin_slot(k)], zn = zw[fft::bin_slot((DN_N - k) & (DN_N - 1))];
                float ar, ai, br, bi;
                st_split(zf, zn, ar, ai, br, bi);
                const float ma = dn_mag(ar, ai), mb = dn_mag(br, bi);
                const float da = ma - bs[n1], db = mb - bs[n1];
                float ga = da > 0.f ? da / ma : 0.f;
                float gb = (vb && db > 0.f) ? db / mb : 0.f;
                if (GATE) {                                  // the floor under the gain; the zero partner of an unpaired last frame keeps gain 0
                    ga = fmaxf(ga, floor);
                    gb = vb ? fmaxf(gb, floor) : 0.f;
                }
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

// ---- efts_noise_profile
constexpr int NP_RUN = 16, NP_WAVES = 4, NP_THREADS = 64 * NP_WAVES;     // frames per run (even: a run begins with a pair); waves per workgroup
static_assert(NP_RUN % 2 == 0, "a run begins on a pair of frames");

// launch 1: one wave per frame
template <typename S>
__global__ __launch_bounds__(NP_THREADS) void np_energy_kernel(const S* __restrict__ audio, long ld, const int* __restrict__ lengths, int max_len,
                                                               const float* __restrict__ window, float pcm_scale, double* __restrict__ energy, int T_max) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = st_len(lengths, b, max_len), T = st_frames(len, DN_N, DN_HOP);
    const int t = blockIdx.x * NP_WAVES + wave;
    if (t >= T) return;
    const S* x = audio + (long)b * ld;
    const int s0 = t * DN_HOP - DN_N / 2;
    const bool inside = s0 >= 0 && s0 + DN_N <= len;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int n = 64 * j + lane;
        const float v = window[n] * pcm_sample(x, inside ? s0 + n : st_reflect(s0 + n, len), pcm_scale);
        s = fma((double)v, (double)v, s);
    }
    s = wave_sum(s);
    if (lane == 0) energy[(long)b * T_max + t] = s;
}

// launch 2: one workgroup per item, on the energies alone
__global__ __launch_bounds__(NP_THREADS) void np_select_kernel(const int* __restrict__ lengths, int max_len, double r, const double* __restrict__ energy,
                                                               int T_max, int R_max, int* __restrict__ flags, int* __restrict__ run_count,
                                                               int* __restrict__ noise_frames, int* __restrict__ frames, double* __restrict__ noise_db) {
    __shared__ double s_m[NP_WAVES], s_s[NP_WAVES];
    __shared__ int s_k[NP_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = st_frames(st_len(lengths, b, max_len), DN_N, DN_HOP);
    const double* e = energy + (long)b * T_max;
    double m = 0.0;
    for (int t = tid; t < T; t += NP_THREADS) m = fmax(m, e[t]);
    m = wave_max(m);
    if (lane == 0) s_m[wave] = m;
    __syncthreads();
    const double e_max = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
    // frame t is a noise frame iff e[t] r < e_max: one multiply, one strict compare (an all-zero item has none)
    int k = 0;
    double sum = 0.0;
    for (int t = tid; t < T; t += NP_THREADS) {
        const double v = e[t];
        const int f = v * r < e_max ? 1 : 0;
        flags[(long)b * T_max + t] = f;
        if (f) { k += 1; sum = sum + v; }
    }
    // the runs' counts, from the same compare on the same energies
    for (int q = tid; q < (T + NP_RUN - 1) / NP_RUN; q += NP_THREADS) {
        int c = 0;
        for (int t = q * NP_RUN; t < min(T, (q + 1) * NP_RUN); ++t) c += e[t] * r < e_max ? 1 : 0;
        run_count[(long)b * R_max + q] = c;
    }
    k = wave_sum(k);
    sum = wave_sum(sum);
    if (lane == 0) { s_k[wave] = k; s_s[wave] = sum; }
    __syncthreads();
    if (tid == 0) {
        const int K = s_k[0] + s_k[1] + s_k[2] + s_k[3];
        const double total = ((s_s[0] + s_s[1]) + s_s[2]) + s_s[3];
        noise_frames[b] = K;
        frames[b] = T;
        noise_db[b] = K > 0 ? 10.0 * log10(total / (double)K / e_max) : __longlong_as_double(0x7ff8000000000000LL);
    }
}

// launch 3: one wave per run of NP_RUN frames
template <typename S>
__global__ __launch_bounds__(NP_THREADS) void np_accum_kernel(const S* __restrict__ audio, long ld, const int* __restrict__ lengths, int max_len,
                                                              const float* __restrict__ window, float pcm_scale, const int* __restrict__ flags,
                                                              const int* __restrict__ run_count, int T_max, int R_max, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) cf zs[NP_WAVES][16 * fft::PITCH];
    __shared__ cf tw1s[15][64];
    __shared__ cf tw2s[4][16];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = st_len(lengths, b, max_len), T = st_frames(len, DN_N, DN_HOP);
    const int R = (T + NP_RUN - 1) / NP_RUN;
    const int* rc = run_count + (long)b * R_max;
    int any = 0;                                         // (uniform in the workgroup)
#pragma unroll
    for (int w = 0; w < NP_WAVES; ++w) {
        const int q = blockIdx.x * NP_WAVES + w;
        if (q < R) any |= rc[q];
    }
    if (!any) return;
    fft::fill_twiddles<NP_THREADS>(tw1s, tw2s);
    __syncthreads();                                     // (the only barrier: from here on a wave is on its own)
    const int run = blockIdx.x * NP_WAVES + wave;
    if (run >= R || rc[run] == 0) return;
    const S* x = audio + (long)b * ld;
    const int* fl = flags + (long)b * T_max;
    cf* zw = zs[wave];
    float win[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1) win[n1] = window[64 * n1 + lane];
    double acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = 0.0;
    for (int t0 = run * NP_RUN; t0 < min(T, (run + 1) * NP_RUN); t0 += 2) {
        const bool vb = t0 + 1 < T;
        const bool fa = fl[t0] != 0, fb = vb && fl[t0 + 1] != 0;
        if (!fa && !fb) continue;                        // (uniform in the wave)
        float sm[20];
        st_load_pair20(x, pcm_scale, t0 * DN_HOP - DN_N / 2, len, lane, sm);
        cf v[16];
        st_pair_values(sm, win, vb, v);
        fft::fft1024(v, zw, tw1s, tw2s, lane);
#pragma unroll
        for (int j = 0; j < 9; ++j) {                    // bins 64 j + lane; j = 8: bin 512, in every lane alike
            const int k = j < 8 ? 64 * j + lane : DN_N / 2;
            const cf zf = zw[fft::bin_slot(k)], zn = zw[fft::bin_slot((DN_N - k) & (DN_N - 1))];
            float ar, ai, br, bi;
            st_split(zf, zn, ar, ai, br, bi);
            if (fa) acc[j] = acc[j] + (double)dn_mag(ar, ai);
            if (fb) acc[j] = acc[j] + (double)dn_mag(br, bi);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the next transform overwrites zw
    }
    double* row = partial + ((long)b * R_max + run) * (DN_N / 2 + 1);
#pragma unroll
    for (int j = 0; j < 8; ++j) row[64 * j + lane] = acc[j];
    if (lane == 0) row[DN_N / 2] = acc[8];
}

// launch 4: one workgroup per item adds the runs' rows in ascending order
__global__ __launch_bounds__(NP_THREADS) void np_reduce_kernel(const int* __restrict__ lengths, int max_len, int min_frames, const int* __restrict__ run_count,
                                                               const int* __restrict__ noise_frames, int R_max, const double* __restrict__ partial,
                                                               float* __restrict__ profile, long ld_profile) {
    const int b = blockIdx.x;
    const int T = st_frames(st_len(lengths, b, max_len), DN_N, DN_HOP);
    const int R = (T + NP_RUN - 1) / NP_RUN, K = noise_frames[b];
    const int* rc = run_count + (long)b * R_max;
    const bool keep = K > 0 && K >= min_frames;
    for (int f = threadIdx.x; f <= DN_N / 2; f += NP_THREADS) {
        double s = 0.0;
        if (keep)
            for (int q = 0; q < R; ++q)
                if (rc[q] != 0) s = s + partial[((long)b * R_max + q) * (DN_N / 2 + 1) + f];
        profile[(long)b * ld_profile + f] = keep ? (float)(s / (double)K) : 0.f;
    }
}

struct np_layout { int64_t T_max, R_max, energy, flags, runs, partial, bytes; };
static np_layout np_workspace(int32_t B, int32_t max_len) {
    np_layout w;
    w.T_max = 1 + max_len / DN_HOP;
    w.R_max = (w.T_max + NP_RUN - 1) / NP_RUN;
    w.energy = 0;
    w.flags = w.energy + efts_round16((int64_t)B * w.T_max * 8);
    w.runs = w.flags + efts_round16((int64_t)B * w.T_max * 4);
    w.partial = w.runs + efts_round16((int64_t)B * w.R_max * 4);
    w.bytes = w.partial + efts_round16((int64_t)B * w.R_max * (DN_N / 2 + 1) * 8);
    return w;
}

template <typename S>
static void np_launch(const S* audio, long ld, const int32_t* lengths, int32_t max_len, const float* window, float pcm_scale, double r, int32_t min_frames,
                      float* profile, long ld_profile, int32_t* noise_frames, int32_t* frames, double* noise_db, char* ws, int32_t B, hipStream_t st) {
    const np_layout w = np_workspace(B, max_len);
    double* energy = (double*)(ws + w.energy);
    int* flags = (int*)(ws + w.flags);
    int* runs = (int*)(ws + w.runs);
    double* partial = (double*)(ws + w.partial);
    const int T_max = (int)w.T_max, R_max = (int)w.R_max;
    hipLaunchKernelGGL(np_energy_kernel<S>, dim3((unsigned)((T_max + NP_WAVES - 1) / NP_WAVES), (unsigned)B), dim3(NP_THREADS), 0, st, audio, ld, lengths, max_len,
                       window, pcm_scale, energy, T_max);
    hipLaunchKernelGGL(np_select_kernel, dim3((unsigned)B), dim3(NP_THREADS), 0, st, lengths, max_len, r, energy, T_max, R_max, flags, runs, noise_frames, frames,
                       noise_db);
    hipLaunchKernelGGL(np_accum_kernel<S>, dim3((unsigned)((R_max + NP_WAVES - 1) / NP_WAVES), (unsigned)B), dim3(NP_THREADS), 0, st, audio, ld, lengths, max_len,
                       window, pcm_scale, flags, runs, T_max, R_max, partial);
    hipLaunchKernelGGL(np_reduce_kernel, dim3((unsigned)B), dim3(NP_THREADS), 0, st, lengths, max_len, min_frames, runs, noise_frames, R_max, partial, profile,
                       ld_profile);
}

}  // namespace efts

using namespace efts;

extern "C" int64_t efts_denoise_workspace_bytes(int32_t, int32_t) {
    return 0;                                            // the overlap-add runs in registers: nothing is kept in memory, whatever the arguments
}

extern "C" int efts_denoise(const float* audio, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window, const float* bias,
                            float strength, float* out, int64_t ld_out, int32_t* frames, void* workspace, int64_t workspace_bytes, int32_t B,
                            void* stream) {
    if (const char* why = efts_audio_bad_shape(B, max_len)) return efts_fail(EFTS_EINVAL, "efts_denoise: %s", why);
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
    hipLaunchKernelGGL((denoise_kernel<float, false>), dim3((unsigned)((ld_out + per - 1) / per), (unsigned)B), dim3(64 * DN_WAVES), 0, (hipStream_t)stream, audio,
                       (long)ld, lengths, max_len, window, bias, 0L, strength, 0.f, 1.f, (const int*)nullptr, out, (long)ld_out, frames);
    return efts_check_launch("efts_denoise");
}

extern "C" int efts_spectral_gate(const void* audio, int32_t pcm16, float pcm_scale, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window,
                                  const float* profile, int64_t ld_profile, float strength, float floor, const int32_t* bypass, float* out, int64_t ld_out,
                                  int32_t* frames, int32_t B, void* stream) {
    const char* who = "efts_spectral_gate";
    if (const char* why = efts_audio_bad_shape(B, max_len)) return efts_fail(EFTS_EINVAL, "%s: %s", who, why);
    if (ld < max_len || ld_out < max_len) return efts_fail(EFTS_EINVAL, "%s: a leading dimension is smaller than the longest item", who);
    if (ld_out > 0x7fffffffLL) return efts_fail(EFTS_EINVAL, "%s: ld_out must stay below 2^31 (every sample of a row is written)", who);
    if (ld_profile != 0 && ld_profile < DN_N / 2 + 1) return efts_fail(EFTS_EINVAL, "%s: ld_profile must be 0 (one shared row) or at least 513", who);
    if (!(strength >= 0.f) || !std::isfinite(strength)) return efts_fail(EFTS_EINVAL, "%s: the strength must be a finite number >= 0", who);
    if (!(floor >= 0.f && floor <= 1.f)) return efts_fail(EFTS_EINVAL, "%s: the floor must lie in 0 .. 1", who);
    if (pcm16 && (!(pcm_scale > 0.f) || !std::isfinite(pcm_scale))) return efts_fail(EFTS_EINVAL, "%s: pcm_scale must be a positive number", who);
    if (!audio || !lengths || !window || !profile || !out || !frames) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    const int64_t esz = pcm16 ? 2 : 4;
    if (((uintptr_t)audio % esz) || ((uintptr_t)lengths & 3) || ((uintptr_t)window & 3) || ((uintptr_t)profile & 3) || ((uintptr_t)out & 3) ||
        ((uintptr_t)frames & 3) || ((uintptr_t)bypass & 3))
        return efts_fail(EFTS_EINVAL, "%s: a pointer is not aligned to its element", who);
    const uintptr_t a0 = (uintptr_t)audio, a1 = a0 + (uintptr_t)(((int64_t)(B - 1) * ld + max_len) * esz);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((int64_t)B * ld_out * 4);
    if (a0 < o1 && o0 < a1) return efts_fail(EFTS_EINVAL, "%s: out overlaps audio (the frames of a hop read samples of its neighbours)", who);
    const int64_t per = (int64_t)DN_WAVES * DN_RUN_SAMPLES;
    const dim3 grid((unsigned)((ld_out + per - 1) / per), (unsigned)B);
    if (pcm16)
        hipLaunchKernelGGL((denoise_kernel<short, true>), grid, dim3(64 * DN_WAVES), 0, (hipStream_t)stream, (const short*)audio, (long)ld, lengths, max_len, window,
                           profile, (long)ld_profile, strength, floor, pcm_scale, bypass, out, (long)ld_out, frames);
    else
        hipLaunchKernelGGL((denoise_kernel<float, true>), grid, dim3(64 * DN_WAVES), 0, (hipStream_t)stream, (const float*)audio, (long)ld, lengths, max_len, window,
                           profile, (long)ld_profile, strength, floor, 1.f, bypass, out, (long)ld_out, frames);
    return efts_check_launch(who);
}

extern "C" int64_t efts_noise_profile_workspace_bytes(int32_t B, int32_t max_len) {
    if (efts_audio_bad_shape(B, max_len)) return 0;
    return np_workspace(B, max_len).bytes;
}

extern "C" int efts_noise_profile(const void* audio, int32_t pcm16, float pcm_scale, int64_t ld, const int32_t* lengths, int32_t max_len, const float* window,
                                  double r, int32_t min_frames, float* profile, int64_t ld_profile, int32_t* noise_frames, int32_t* frames, double* noise_db,
                                  void* workspace, int64_t workspace_bytes, int32_t B, void* stream) {
    const char* who = "efts_noise_profile";
    if (const char* why = efts_audio_bad_shape(B, max_len)) return efts_fail(EFTS_EINVAL, "%s: %s", who, why);
    if (ld < max_len) return efts_fail(EFTS_EINVAL, "%s: a leading dimension is smaller than the longest item", who);
    if (ld_profile < DN_N / 2 + 1) return efts_fail(EFTS_EINVAL, "%s: ld_profile must be at least 513", who);
    if (!(r > 1.0) || !std::isfinite(r)) return efts_fail(EFTS_EINVAL, "%s: the threshold ratio r = 10^(top_db / 10) must be a finite number > 1", who);
    if (min_frames < 1) return efts_fail(EFTS_EINVAL, "%s: min_frames must be >= 1", who);
    if (pcm16 && (!(pcm_scale > 0.f) || !std::isfinite(pcm_scale))) return efts_fail(EFTS_EINVAL, "%s: pcm_scale must be a positive number", who);
    if (!audio || !lengths || !window || !profile || !noise_frames || !frames || !noise_db || !workspace) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (((uintptr_t)audio % (pcm16 ? 2 : 4)) || ((uintptr_t)lengths & 3) || ((uintptr_t)window & 3) || ((uintptr_t)profile & 3) || ((uintptr_t)noise_frames & 3) ||
        ((uintptr_t)frames & 3) || ((uintptr_t)noise_db & 7) || ((uintptr_t)workspace & 15))
        return efts_fail(EFTS_EINVAL, "%s: a pointer is not aligned to its element (the workspace: to 16 bytes)", who);
    if (workspace_bytes < efts_noise_profile_workspace_bytes(B, max_len))
        return efts_fail(EFTS_EINVAL, "%s: the workspace is smaller than efts_noise_profile_workspace_bytes asks for", who);
    if (pcm16)
        np_launch<short>((const short*)audio, (long)ld, lengths, max_len, window, pcm_scale, r, min_frames, profile, (long)ld_profile, noise_frames, frames, noise_db,
                         (char*)workspace, B, (hipStream_t)stream);
    else
        np_launch<float>((const float*)audio, (long)ld, lengths, max_len, window, 1.f, r, min_frames, profile, (long)ld_profile, noise_frames, frames, noise_db,
                         (char*)workspace, B, (hipStream_t)stream);
    return efts_check_launch(who);
}
