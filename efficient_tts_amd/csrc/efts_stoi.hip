// efts_stoi.hip -- short-time objective intelligibility of a processed signal y against the clean signal x, both at 10 000 Hz and aligned
// sample by sample: STOI (Taal et al. 2011) and ESTOI (Jensen and Taal 2016) as the authors' Matlab code defines them
// (include/efts_abi.h has the definition, the order of every sum included; efficient_tts_amd/stoi.py is the host side).
//
//   stoi_energy_kernel  : e[f] = sum of (w x)^2 over frame f of x (256 samples, hop 128), one wave per frame, fp32 in one order.
//   stoi_select_kernel  : one workgroup per item: e_max, the keep flags e[f] 10^4 > e_max (compared in fp64), their exclusive scan ->
//                         the list k_0 < k_1 < .. of kept frames and K; writes frames, kept and segments.
//   stoi_spectra_kernel : a group of 32 lanes takes spectral frame t of the compacted signals: it puts w * xs and w * ys together from the
//                         kept frames k_(t-1) (second half), k_t and k_(t+1) (first half) -- the compacted signals never exist --, runs
//                         them as ONE complex 512-point transform z = xs-frame + i ys-frame (efts_fft.h, plan<16, 2>: two transforms per
//                         wave), takes the two spectra apart by conjugate symmetry and sums the 15 one-third-octave bands in bin order:
//                         X[b][t][16], Y[b][t][16] in fp32 (slot 15 is 0).  No spectrum goes to memory.
//   stoi_segment_kernel : half a wave per segment of 30 frames, lane n = frame n with its 15 + 15 band values in registers, all in fp64:
//                         sums over the frames are xor trees over the 32 lanes (lanes 30, 31 hold 0), sums over the bands run in the lane
//                         in ascending order.  The two sums of a segment go to the workspace.
//   stoi_reduce_kernel  : per item the segments' sums in segment order (fp64) and the two divisions; NaN where there is no segment.
// No atomics, nothing read back by the host, no launch geometry that depends on device data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "efts_internal.h"
#include "efts_fft.h"
#include "efts_stft_frame.h"

// every product and sum below is rounded as written (the fused ones are written as fmaf / fma): a sum over lanes must leave the same bits in
// every lane, which a product contracted into one lane's addition would break
#pragma clang fp contract(off)

namespace efts {

using fft::cf;

constexpr int SI_FRAME = 256, SI_HOP = 128, SI_BANDS = 15, SI_SEG = 30;
constexpr int SI_ROW = 16;                                   // floats per row of X and Y: the 15 bands and one zero
constexpr int SI_E_WAVES = 4, SI_E_ITER = 8;                 // energies: frames per workgroup = 32
constexpr int SI_S_GROUPS = 8, SI_S_ITER = 4;                // spectra: groups of 32 lanes per workgroup, frames per group
constexpr int SI_G_GROUPS = 8, SI_G_ITER = 1;                // segments: half-waves per workgroup, segments per half-wave (a segment is one long
                                                             // chain of dependent lane exchanges: more waves hide it, more turns do not)
constexpr int SI_CHUNK = 512;                                // segments per step of the last sum
typedef fft::plan<16, 2> si_plan;

__constant__ int si_lo[16] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 0};
__constant__ int si_hi[16] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219, 0};

__host__ __device__ __forceinline__ int si_frames(int len) { return len >= SI_FRAME ? (len - SI_FRAME) / SI_HOP + 1 : 0; }

__global__ __launch_bounds__(64 * SI_E_WAVES) void stoi_energy_kernel(const float* __restrict__ x, long ldx, const int* __restrict__ lengths, int max_len,
                                                                       const float* __restrict__ window, float* __restrict__ e, int F_max) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int F = si_frames(st_len(lengths, b, max_len));
    const int f0 = (blockIdx.x * SI_E_WAVES + wave) * SI_E_ITER;
    if (f0 >= F) return;
    float w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = window[lane + 64 * j];
    const float* xb = x + (long)b * ldx;
    for (int f = f0; f < min(f0 + SI_E_ITER, F); ++f) {
        const float* p = xb + (long)f * SI_HOP + lane;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = w[j] * p[64 * j];
            s = fmaf(v, v, s);
        }
        s = wave_sum(s);
        if (lane == 0) e[(long)b * F_max + f] = s;
    }
}

__global__ __launch_bounds__(256) void stoi_select_kernel(const float* __restrict__ e, const int* __restrict__ lengths, int max_len, int F_max,
                                                           int* __restrict__ klist, int* __restrict__ frames, int* __restrict__ kept, int* __restrict__ segments) {
    __shared__ float wm[4];
    __shared__ int wt[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = si_frames(st_len(lengths, b, max_len));
    const float* eb = e + (long)b * F_max;
    int* kb = klist + (long)b * F_max;
    float m = 0.f;                                           // (energies are >= 0)
    for (int f = tid; f < F; f += 256) m = fmaxf(m, eb[f]);
    m = wave_max(m);
    if (lane == 0) wm[wave] = m;
    __syncthreads();
    const double e_max = (double)fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    int base = 0;
    for (int c0 = 0; c0 < F; c0 += 256) {                    // (F is uniform in the workgroup)
        const int f = c0 + tid;
        const bool keep = f < F && (double)eb[f] * 1e4 > e_max;
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();                                     // (the previous turn's reads of wt)
        if (lane == 0) wt[wave] = __popcll(mask);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { off += i < wave ? wt[i] : 0; total += wt[i]; }
        if (keep) kb[base + off + before] = f;
        base += total;
    }
    if (tid == 0) {
        frames[b] = F;
        kept[b] = base;
        segments[b] = base > SI_SEG ? base - SI_SEG : 0;
    }
}

__global__ __launch_bounds__(32 * SI_S_GROUPS) void stoi_spectra_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ y, long ldy,
                                                                         const int* __restrict__ lengths, int max_len, const float* __restrict__ window,
                                                                         const int* __restrict__ klist, const int* __restrict__ kept, int F_max,
                                                                         float* __restrict__ X, float* __restrict__ Y, int T_max) {
    __shared__ __attribute__((aligned(16))) cf zs[SI_S_GROUPS][si_plan::BUF];
    __shared__ cf tw1s[15][32];
    __shared__ cf tw2s[2][16];
    const int b = blockIdx.y, g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int F = si_frames(st_len(lengths, b, max_len));
    const int T = min(max(kept[b], 0), F) - 1;               // spectral frames: K - 1
    const int t0 = blockIdx.x * (SI_S_GROUPS * SI_S_ITER);
    if (t0 >= T) return;                                     // (uniform) nothing of this item here
    fft::fill_twiddles_mp<16, 2, 32 * SI_S_GROUPS>(tw1s, tw2s);
    __syncthreads();                                         // (the only barrier: from here on a group is on its own)
    cf* zw = zs[g];
    float w[8];
#pragma unroll
    for (int n1 = 0; n1 < 8; ++n1) w[n1] = window[32 * n1 + l];
    const float* xb = x + (long)b * ldx;
    const float* yb = y + (long)b * ldy;
    const int* kb = klist + (long)b * F_max;
    for (int it = 0; it < SI_S_ITER; ++it) {
        const int t = t0 + it * SI_S_GROUPS + g;
        if (t >= T) continue;
        // the kept frames around t, as sample offsets (clamped into the item: a frame index is at most F - 1, so 128 k + 255 < len)
        const long s1 = (long)min(max(kb[t], 0), F - 1) * SI_HOP, s2 = (long)min(max(kb[t + 1], 0), F - 1) * SI_HOP;
        const long s0 = t > 0 ? (long)min(max(kb[t - 1], 0), F - 1) * SI_HOP : 0;
        const bool older = t > 0;                            // frame k_(t-1) is absent at t = 0
        cf v[16];
#pragma unroll
        for (int n1 = 0; n1 < 4; ++n1) {                     // i = 32 n1 + l < 128: the second half of k_(t-1), then the first half of k_t
            const int i = 32 * n1 + l;
            const float ox = older ? w[n1 + 4] * xb[s0 + 128 + i] : 0.f, oy = older ? w[n1 + 4] * yb[s0 + 128 + i] : 0.f;
            v[n1] = cf{w[n1] * fmaf(w[n1], xb[s1 + i], ox), w[n1] * fmaf(w[n1], yb[s1 + i], oy)};
        }
#pragma unroll
        for (int n1 = 4; n1 < 8; ++n1) {                     // i >= 128: the second half of k_t, then the first half of k_(t+1)
            const int i = 32 * n1 + l;
            const float ox = w[n1] * xb[s1 + i], oy = w[n1] * yb[s1 + i];
            v[n1] = cf{w[n1] * fmaf(w[n1 - 4], xb[s2 + i - 128], ox), w[n1] * fmaf(w[n1 - 4], yb[s2 + i - 128], oy)};
        }
#pragma unroll
        for (int n1 = 8; n1 < 16; ++n1) v[n1] = cf{0.f, 0.f};
        fft::fft_group<16, 2>(v, zw, tw1s, tw2s, l);
        // lane j sums band j of x, lane 16 + j band j of y, in bin order; lanes 15 and 31 write the zero of slot 15
        const int j = l & 15;
        const bool second = l >= 16;
        float acc = 0.f;
        for (int f = si_lo[j]; f < si_hi[j]; ++f) {
            const cf zf = zw[si_plan::slot(f)], zn = zw[si_plan::slot(512 - f)];
            float ar, ai, br, bi;
            st_split(zf, zn, ar, ai, br, bi);
            const float re = second ? br : ar, im = second ? bi : ai;
            acc += fmaf(re, re, im * im);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the next transform overwrites zw
        (second ? Y : X)[((long)b * T_max + t) * SI_ROW + j] = sqrtf(acc);
    }
}

// the sum over the 32 lanes of a half-wave: every lane ends with the same bits
__device__ __forceinline__ double si_sum32(double v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(32 * SI_G_GROUPS) void stoi_segment_kernel(const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ segments,
                                                                         int T_max, int M_max, double* __restrict__ seg) {
    const int b = blockIdx.y, g = threadIdx.x >> 5, n = threadIdx.x & 31;
    const int M = min(max(segments[b], 0), M_max);
    const int m0 = (blockIdx.x * SI_G_GROUPS + g) * SI_G_ITER;
    constexpr double EPS = 2.220446049250313e-16, CLIP = 6.623413251903491;           // 2^-52; 1 + 10^(15 / 20)
    const bool act = n < SI_SEG;
    for (int m = m0; m < min(m0 + SI_G_ITER, M); ++m) {      // (uniform in the half-wave)
        double xv[SI_BANDS], yv[SI_BANDS];
        if (act) {
            const float4* px = (const float4*)(X + ((long)b * T_max + m + n) * SI_ROW);
            const float4* py = (const float4*)(Y + ((long)b * T_max + m + n) * SI_ROW);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 a = px[q], c = py[q];
                xv[4 * q] = a.x; xv[4 * q + 1] = a.y; xv[4 * q + 2] = a.z; if (q < 3) xv[4 * q + 3] = a.w;
                yv[4 * q] = c.x; yv[4 * q + 1] = c.y; yv[4 * q + 2] = c.z; if (q < 3) yv[4 * q + 3] = c.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < SI_BANDS; ++j) xv[j] = yv[j] = 0.0;
        }
        // STOI per band; the rows of ESTOI (a band over the 30 frames) on the way
        double d_sum = 0.0;
        double xr[SI_BANDS], yr[SI_BANDS];
#pragma unroll
        for (int j = 0; j < SI_BANDS; ++j) {
            const double xn = sqrt(si_sum32(xv[j] * xv[j])), yn = sqrt(si_sum32(yv[j] * yv[j]));
            const double c = xn / (yn + EPS);
            const double yp = fmin(c * yv[j], xv[j] * CLIP);
            const double mx = si_sum32(xv[j]) / 30.0, my = si_sum32(yv[j]) / 30.0, mp = si_sum32(yp) / 30.0;
            const double xc = act ? xv[j] - mx : 0.0, yc = act ? yv[j] - my : 0.0, pc = act ? yp - mp : 0.0;
            const double xcn = sqrt(si_sum32(xc * xc)), ycn = sqrt(si_sum32(yc * yc)), pcn = sqrt(si_sum32(pc * pc));
            xr[j] = xc / (xcn + EPS);
            yr[j] = yc / (ycn + EPS);
            d_sum += si_sum32(xr[j] * (pc / (pcn + EPS)));
        }
        // ESTOI: the columns (a frame over the 15 bands) of the row-normalised blocks, in the lane
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int j = 0; j < SI_BANDS; ++j) { sx += xr[j]; sy += yr[j]; }
        const double cx = sx / 15.0, cy = sy / 15.0;
        double qx = 0.0, qy = 0.0;
#pragma unroll
        for (int j = 0; j < SI_BANDS; ++j) {
            xr[j] -= cx; yr[j] -= cy;
            qx = fma(xr[j], xr[j], qx); qy = fma(yr[j], yr[j], qy);
        }
        const double ix = sqrt(qx) + EPS, iy = sqrt(qy) + EPS;
        double dot = 0.0;
#pragma unroll
        for (int j = 0; j < SI_BANDS; ++j) dot = fma(xr[j] / ix, yr[j] / iy, dot);
        const double e_sum = si_sum32(act ? dot : 0.0);
        if (n == 0) {
            double* o = seg + ((long)b * M_max + m) * 2;
            o[0] = d_sum; o[1] = e_sum;
        }
    }
}

__global__ __launch_bounds__(64) void stoi_reduce_kernel(const double* __restrict__ seg, const int* __restrict__ segments, int M_max,
                                                          double* __restrict__ stoi, double* __restrict__ estoi) {
    __shared__ double s[2 * SI_CHUNK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int M = min(max(segments[b], 0), M_max);
    const double* p = seg + (long)b * M_max * 2;
    double acc = 0.0;
    for (int c0 = 0; c0 < M; c0 += SI_CHUNK) {               // (M is uniform in the workgroup)
        const int n = min(SI_CHUNK, M - c0);
        __syncthreads();
        for (int i = tid; i < 2 * n; i += 64) s[i] = p[2L * c0 + i];
        __syncthreads();
        if (tid < 2)
            for (int i = 0; i < n; ++i) acc += s[2 * i + tid];
    }
    if (tid < 2) {
        double r = NAN;                                      // no segment: K <= 30, F = 0 or an all-zero x
        if (M > 0) r = acc / ((tid == 0 ? 15.0 : 30.0) * (double)M);
        (tid == 0 ? stoi : estoi)[b] = r;
    }
}

struct si_layout { int64_t F_max, T_max, M_max, e, klist, X, Y, seg, bytes; };

static si_layout si_make_layout(int32_t B, int32_t max_len) {
    si_layout L;
    L.F_max = si_frames(max_len);
    L.T_max = L.F_max > 1 ? L.F_max - 1 : 0;
    L.M_max = L.T_max > SI_SEG - 1 ? L.T_max - (SI_SEG - 1) : 0;
    int64_t at = 0;
    L.e = at;     at += efts_round16((int64_t)B * L.F_max * 4);
    L.klist = at; at += efts_round16((int64_t)B * L.F_max * 4);
    L.X = at;     at += efts_round16((int64_t)B * L.T_max * SI_ROW * 4);
    L.Y = at;     at += efts_round16((int64_t)B * L.T_max * SI_ROW * 4);
    L.seg = at;   at += efts_round16((int64_t)B * L.M_max * 2 * 8);
    L.bytes = at > 16 ? at : 16;
    return L;
}

}  // namespace efts

using namespace efts;

extern "C" int64_t efts_stoi_workspace_bytes(int32_t B, int32_t max_len) {
    if (efts_audio_bad_shape(B, max_len)) return 0;
    return si_make_layout(B, max_len).bytes;
}

extern "C" int efts_stoi(const float* x, int64_t ldx, const float* y, int64_t ldy, const int32_t* lengths, int32_t max_len, const float* window,
                         double* stoi, double* estoi, int32_t* frames, int32_t* kept, int32_t* segments, void* workspace, int64_t workspace_bytes,
                         int32_t B, void* stream) {
    if (const char* why = efts_audio_bad_shape(B, max_len)) return efts_fail(EFTS_EINVAL, "efts_stoi: %s", why);
    if (ldx < max_len || ldy < max_len) return efts_fail(EFTS_EINVAL, "efts_stoi: a leading dimension is smaller than the longest item");
    const si_layout L = si_make_layout(B, max_len);
    if (workspace_bytes < L.bytes) return efts_fail(EFTS_EINVAL, "efts_stoi: the workspace is smaller than efts_stoi_workspace_bytes asks for");
    if (!x || !y || !lengths || !window || !stoi || !estoi || !frames || !kept || !segments || !workspace) return efts_fail(EFTS_EINVAL, "efts_stoi: null pointer");
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)lengths & 3) || ((uintptr_t)window & 3) || ((uintptr_t)stoi & 7) || ((uintptr_t)estoi & 7) ||
        ((uintptr_t)frames & 3) || ((uintptr_t)kept & 3) || ((uintptr_t)segments & 3) || ((uintptr_t)workspace & 15))
        return efts_fail(EFTS_EINVAL, "efts_stoi: a pointer is not aligned to its element (the workspace: to 16 bytes)");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* e = (float*)(ws + L.e);
    int* klist = (int*)(ws + L.klist);
    float* X = (float*)(ws + L.X);
    float* Y = (float*)(ws + L.Y);
    double* seg = (double*)(ws + L.seg);
    const int F_max = (int)L.F_max, T_max = (int)L.T_max, M_max = (int)L.M_max;
    if (F_max > 0) {
        constexpr int per = SI_E_WAVES * SI_E_ITER;
        hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((F_max + per - 1) / per), (unsigned)B), dim3(64 * SI_E_WAVES), 0, st, x, (long)ldx, lengths, max_len,
                           window, e, F_max);
    }
    hipLaunchKernelGGL(stoi_select_kernel, dim3((unsigned)B), dim3(256), 0, st, (const float*)e, lengths, max_len, F_max, klist, frames, kept, segments);
    if (M_max > 0) {                                         // (without a possible segment the spectra have no reader)
        constexpr int per = SI_S_GROUPS * SI_S_ITER, per_seg = SI_G_GROUPS * SI_G_ITER;
        hipLaunchKernelGGL(stoi_spectra_kernel, dim3((unsigned)((T_max + per - 1) / per), (unsigned)B), dim3(32 * SI_S_GROUPS), 0, st, x, (long)ldx, y, (long)ldy,
                           lengths, max_len, window, (const int*)klist, (const int*)kept, F_max, X, Y, T_max);
        hipLaunchKernelGGL(stoi_segment_kernel, dim3((unsigned)((M_max + per_seg - 1) / per_seg), (unsigned)B), dim3(32 * SI_G_GROUPS), 0, st, (const float*)X,
                           (const float*)Y, (const int*)segments, T_max, M_max, seg);
    }
    hipLaunchKernelGGL(stoi_reduce_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)seg, (const int*)segments, M_max, stoi, estoi);
    return efts_check_launch("efts_stoi");
}
