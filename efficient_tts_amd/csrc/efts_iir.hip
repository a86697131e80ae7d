// efts_iir.hip -- a cascade of up to four second-order sections applied to every item of a padded batch, in fp64, with the exact filter state
// carried from segment to segment (include/efts_abi.h has the definition; efficient_tts_amd/iir.py is the host side).  Three launches on
// one stream, no host synchronisation, no allocation, no atomics:
//
//   A  iir_zero_kernel  : one thread per (item, segment of EFTS_IIR_SEGMENT samples) that has a successor inside the item runs the cascade from
//                         zero state over its samples and writes the end state Z to the workspace.
//   B  iir_carry_kernel : one wave per item.  64 segments at a time, lane l holds the end state of segment l given the state at the chunk's
//                         start: a Hillis-Steele scan with the host's M^(2^k), k = 0 .. 5, copied from device memory into LDS once and read
//                         from there at one address per wave.  The state that enters the chunk goes into lane 0 before the scan, the end
//                         state of lane 63 enters the next chunk.  The start state of every segment overwrites its Z.
//   C  iir_out_kernel   : one thread per segment re-runs its samples from its start state and writes the output; zeros behind the length.
//
// In A and C a thread owns a contiguous segment, so across the wave global addresses are EFTS_IIR_SEGMENT samples apart.  A workgroup of one
// wave therefore moves its span of 64 segments through LDS in four tiles of 64 segments x 64 samples: global accesses are 16 bytes per lane
// (int16: 8), 8 lanes on one segment's 128 contiguous bytes, and a tile's row pitch is 65 floats, so that both the four stores of a staged
// group (4 rows x 8 groups per half wave) and the per-lane reads down a row (lane l at l * 65 + j) fall on 32 distinct banks.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "efts_internal.h"

namespace efts {

constexpr int IIR_L = EFTS_IIR_SEGMENT;                    // samples of one thread
constexpr int IIR_KMAX = EFTS_IIR_MAX_SECTIONS;
constexpr int IIR_NMAX = 2 * IIR_KMAX;                     // doubles of one workspace slot: the state of the longest cascade
constexpr int IIR_THREADS = 64;                            // one wave: segments of one workgroup
constexpr int IIR_SPAN = IIR_THREADS * IIR_L;              // samples of one workgroup
constexpr int IIR_T = 64;                                  // samples per segment in one LDS tile
constexpr int IIR_PITCH = IIR_T + 1;                       // floats from one segment's row to the next: odd
constexpr int IIR_LOG = 6;                                 // scan steps over the 64 lanes
static_assert(IIR_L % IIR_T == 0 && IIR_T == 64 && IIR_THREADS == 64, "the tile mapping below is written for 64 x 64");

struct iir_coef { double c[IIR_KMAX][5]; };                // b0, b1, b2, a1, a2 per section

// one sample through the cascade: transposed direct form II, every product folded into an fma in the order of the header
template <int K>
__device__ __forceinline__ double iir_step(const iir_coef& f, double (&s)[2 * K], double x) {
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const double y = fma(f.c[q][0], x, s[2 * q]);
        s[2 * q] = fma(-f.c[q][3], y, fma(f.c[q][1], x, s[2 * q + 1]));
        s[2 * q + 1] = fma(-f.c[q][4], y, f.c[q][2] * x);
        x = y;
    }
    return x;
}

__device__ __forceinline__ float4 iir_load4(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ float4 iir_load4(const short* p, float scale) {
    const short4 v = *(const short4*)p;
    return make_float4((float)v.x * scale, (float)v.y * scale, (float)v.z * scale, (float)v.w * scale);
}
__device__ __forceinline__ float4 iir_load4(const float* p, float) { return iir_load4(p); }
__device__ __forceinline__ float iir_load1(const float* p, float) { return *p; }
__device__ __forceinline__ float iir_load1(const short* p, float scale) { return (float)*p * scale; }

// tile[r * IIR_PITCH + c] = x[span0 + r * IIR_L + t0 + c] for r, c = 0 .. 63; 0 at and behind len, where nothing is read.
// Group g = 0 .. 1023 of four samples: column half g / 512, row (g % 512) / 8, group (g % 8) of the half.
template <typename S>
__device__ __forceinline__ void iir_stage(float* tile, const S* row, bool vec, long span0, int t0, long len, float scale) {
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
        const int g = it * IIR_THREADS + threadIdx.x;
        const int r = (g & 511) >> 3, c = ((g >> 9) << 5) + ((g & 7) << 2);
        const long i = span0 + (long)r * IIR_L + t0 + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vec && i + 4 <= len) {
            v = iir_load4(row + i, scale);
        } else {
            if (i < len) v.x = iir_load1(row + i, scale);
            if (i + 1 < len) v.y = iir_load1(row + i + 1, scale);
            if (i + 2 < len) v.z = iir_load1(row + i + 2, scale);
            if (i + 3 < len) v.w = iir_load1(row + i + 3, scale);
        }
        float* d = tile + r * IIR_PITCH + c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}

// ---- launch A: Z of every segment that has a successor
template <typename S, int K>
__global__ __launch_bounds__(IIR_THREADS) void iir_zero_kernel(const S* __restrict__ in, long ld_in, const int* __restrict__ lengths, iir_coef f,
                                                               float scale, double* __restrict__ ws, long nseg_max) {
    __shared__ float tile[IIR_THREADS * IIR_PITCH];
    const int b = blockIdx.y;
    const long len = min((long)max(lengths[b], 0), ld_in);
    const long span0 = (long)blockIdx.x * IIR_SPAN;
    if (span0 + IIR_L >= len) return;                              // no segment of this span has a successor
    const S* row = in + (long)b * ld_in;
    const bool vec = ((uintptr_t)row % (4 * sizeof(S))) == 0;
    const long seg = (long)blockIdx.x * IIR_THREADS + threadIdx.x;
    double s[2 * K];
#pragma unroll
    for (int i = 0; i < 2 * K; ++i) s[i] = 0.0;
    for (int t0 = 0; t0 < IIR_L; t0 += IIR_T) {
        __syncthreads();                                           // the tile before has been read
        iir_stage(tile, row, vec, span0, t0, len, scale);
        __syncthreads();
        const float* x = tile + threadIdx.x * IIR_PITCH;
#pragma unroll 4
        for (int j = 0; j < IIR_T; ++j) iir_step<K>(f, s, (double)x[j]);
    }
    if ((seg + 1) * IIR_L < len) {
        double* z = ws + ((long)b * nseg_max + seg) * IIR_NMAX;
#pragma unroll
        for (int i = 0; i < 2 * K; ++i) z[i] = s[i];
    }
}

// ---- launch B: the start state of every segment
template <int K>
__global__ __launch_bounds__(IIR_THREADS) void iir_carry_kernel(const int* __restrict__ lengths, long ld_in, const double* __restrict__ powers,
                                                                double* __restrict__ ws, long nseg_max) {
    constexpr int N = 2 * K;
    __shared__ double pw[IIR_LOG][N * N];                          // M^(2^k), row-major
    const int b = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < IIR_LOG * N * N; i += IIR_THREADS) pw[0][i] = powers[i];
    __syncthreads();
    const long len = min((long)max(lengths[b], 0), ld_in);
    const long nseg = (len + IIR_L - 1) / IIR_L;
    double carry[N];                                               // the state at the chunk's start: the same in every lane
#pragma unroll
    for (int i = 0; i < N; ++i) carry[i] = 0.0;
    for (long c0 = 0; c0 < nseg; c0 += IIR_THREADS) {
        const long seg = c0 + lane;
        double* slot = ws + ((long)b * nseg_max + seg) * IIR_NMAX;
        double p[N];
        const bool has_z = (seg + 1) * IIR_L < len;                // launch A wrote this slot
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = has_z ? slot[i] : 0.0;
        // step 0 puts the chunk's start state into lane 0 (the end state of segment c0 is M carry + Z); step k + 1 is step k of the scan, after
        // which p is the end state given the start state of segment seg - 2^(k + 1) + 1.  One rolled loop: the matrix of a step is read from
        // LDS when the step needs it and is not kept in registers across the chunks.
#pragma unroll 1
        for (int step = 0; step <= IIR_LOG; ++step) {
            const int k = step == 0 ? 0 : step - 1, d = 1 << k;
            const double* m = pw[k];
            double v[N], q[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const double up = __shfl_up(p[i], d);
                v[i] = step == 0 ? carry[i] : up;
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {
                double acc = p[i];
#pragma unroll
                for (int j = 0; j < N; ++j) acc = fma(m[i * N + j], v[j], acc);
                q[i] = acc;
            }
            if (step == 0 ? lane == 0 : lane >= d) {
#pragma unroll
                for (int i = 0; i < N; ++i) p[i] = q[i];
            }
        }
        double start[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double up = __shfl_up(p[i], 1);
            start[i] = lane == 0 ? carry[i] : up;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) carry[i] = __shfl(p[i], IIR_THREADS - 1);
        if (seg < nseg) {
#pragma unroll
            for (int i = 0; i < N; ++i) slot[i] = start[i];
        }
    }
}

// ---- launch C: the output
template <typename S, int K>
__global__ __launch_bounds__(IIR_THREADS) void iir_out_kernel(const S* __restrict__ in, long ld_in, const int* __restrict__ lengths, iir_coef f,
                                                              float scale, const double* __restrict__ ws, long nseg_max, float* __restrict__ out,
                                                              long ld_out) {
    __shared__ float tile[IIR_THREADS * IIR_PITCH];
    const int b = blockIdx.y;
    const long len = min((long)max(lengths[b], 0), ld_in);
    const long span0 = (long)blockIdx.x * IIR_SPAN;
    float* orow = out + (long)b * ld_out;
    const bool ovec = ((uintptr_t)orow & 15) == 0;
    if (span0 >= len) {                                            // behind the item: +0.0, nothing read
        const long end = min(span0 + IIR_SPAN, ld_out);
        for (long i = span0 + 4 * threadIdx.x; i < end; i += 4 * IIR_THREADS) {
            if (ovec && i + 4 <= end) *(float4*)(orow + i) = make_float4(0.f, 0.f, 0.f, 0.f);
            else for (int n = 0; n < 4 && i + n < end; ++n) orow[i + n] = 0.f;
        }
        return;
    }
    const S* row = in + (long)b * ld_in;
    const bool vec = ((uintptr_t)row % (4 * sizeof(S))) == 0;
    const long seg = (long)blockIdx.x * IIR_THREADS + threadIdx.x;
    double s[2 * K];
    {
        const bool live = seg * IIR_L < len;                       // launch B wrote this slot
        const double* st = ws + ((long)b * nseg_max + seg) * IIR_NMAX;
#pragma unroll
        for (int i = 0; i < 2 * K; ++i) s[i] = live ? st[i] : 0.0;
    }
    for (int t0 = 0; t0 < IIR_L; t0 += IIR_T) {
        __syncthreads();                                           // the tile before has been stored
        iir_stage(tile, row, vec, span0, t0, len, scale);
        __syncthreads();
        float* x = tile + threadIdx.x * IIR_PITCH;
#pragma unroll 4
        for (int j = 0; j < IIR_T; ++j) x[j] = (float)iir_step<K>(f, s, (double)x[j]);
        __syncthreads();
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {                          // the groups of iir_stage, back to memory
            const int g = it * IIR_THREADS + threadIdx.x;
            const int r = (g & 511) >> 3, c = ((g >> 9) << 5) + ((g & 7) << 2);
            const long i = span0 + (long)r * IIR_L + t0 + c;
            if (i >= ld_out) continue;
            const float* y = tile + r * IIR_PITCH + c;
            const float4 v = make_float4(i < len ? y[0] : 0.f, i + 1 < len ? y[1] : 0.f, i + 2 < len ? y[2] : 0.f, i + 3 < len ? y[3] : 0.f);
            if (ovec && i + 4 <= ld_out) {
                *(float4*)(orow + i) = v;
            } else {
                orow[i] = v.x;
                if (i + 1 < ld_out) orow[i + 1] = v.y;
                if (i + 2 < ld_out) orow[i + 2] = v.z;
                if (i + 3 < ld_out) orow[i + 3] = v.w;
            }
        }
    }
}

static inline int64_t iir_nseg(int64_t max_len) { return (max_len + IIR_L - 1) / IIR_L; }
static inline int64_t iir_nspan(int64_t max_len) { return (max_len + IIR_SPAN - 1) / IIR_SPAN; }

template <typename S, int K>
static void iir_launch_k(const S* in, long ld_in, const int* lengths, const iir_coef& f, const double* powers, float scale, float* out, long ld_out,
                         double* ws, int B, hipStream_t st) {
    const long nseg = iir_nseg(ld_in);
    hipLaunchKernelGGL((iir_zero_kernel<S, K>), dim3((unsigned)iir_nspan(ld_in), (unsigned)B), dim3(IIR_THREADS), 0, st, in, ld_in, lengths, f, scale, ws, nseg);
    hipLaunchKernelGGL((iir_carry_kernel<K>), dim3((unsigned)B), dim3(IIR_THREADS), 0, st, lengths, ld_in, powers, ws, nseg);
    hipLaunchKernelGGL((iir_out_kernel<S, K>), dim3((unsigned)iir_nspan(ld_out), (unsigned)B), dim3(IIR_THREADS), 0, st, in, ld_in, lengths, f, scale,
                       (const double*)ws, nseg, out, ld_out);
}

template <typename S>
static int iir_launch(const S* in, int64_t ld_in, const int32_t* lengths, const double* sos, int32_t K, const double* powers, float scale, float* out,
                      int64_t ld_out, void* workspace, int32_t B, void* stream, const char* who) {
    if (B <= 0 || B > 65535) return efts_fail(EFTS_ESHAPE, "%s: 1 .. 65535 items per launch", who);
    if (ld_in < 1 || ld_in > 0x7fffffffLL - 4 * 2048) return efts_fail(EFTS_ESHAPE, "%s: ld_in must lie in 1 .. 2^31 - 8193", who);
    if (ld_out < ld_in || ld_out > 0x7fffffffLL - 4 * 2048) return efts_fail(EFTS_ESHAPE, "%s: ld_out must lie in ld_in .. 2^31 - 8193", who);
    if (K < 1 || K > IIR_KMAX) return efts_fail(EFTS_ESHAPE, "%s: 1 .. %d sections", who, IIR_KMAX);
    if (!in || !lengths || !sos || !powers || !out || !workspace) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (((uintptr_t)in % sizeof(S)) || ((uintptr_t)lengths & 3) || ((uintptr_t)sos & 7) || ((uintptr_t)powers & 7) || ((uintptr_t)out & 3) ||
        ((uintptr_t)workspace & 15))
        return efts_fail(EFTS_EINVAL, "%s: misaligned pointer (every array to its element, the workspace to 16 bytes)", who);
    if (!std::isfinite(scale) || !(scale > 0.f)) return efts_fail(EFTS_EINVAL, "%s: pcm_scale must be a positive number", who);
    iir_coef f;
    for (int q = 0; q < IIR_KMAX; ++q)
        for (int i = 0; i < 5; ++i) f.c[q][i] = q < K ? sos[q * 5 + i] : 0.0;
    for (int q = 0; q < K; ++q) {
        for (int i = 0; i < 5; ++i)
            if (!std::isfinite(f.c[q][i])) return efts_fail(EFTS_EINVAL, "%s: section %d has a coefficient that is not finite", who, q);
        const double a1 = f.c[q][3], a2 = f.c[q][4];
        if (!(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2))
            return efts_fail(EFTS_EINVAL, "%s: section %d has a pole on or outside the unit circle (|a2| < 1 and |a1| < 1 + a2 are required)", who, q);
    }
    const char* in_lo = (const char*)in;
    const char* in_hi = in_lo + (int64_t)B * ld_in * (int64_t)sizeof(S);
    const char* out_lo = (const char*)out;
    const char* out_hi = out_lo + (int64_t)B * ld_out * 4;
    if (in_lo < out_hi && out_lo < in_hi) return efts_fail(EFTS_EINVAL, "%s: out overlaps in (the input is read twice)", who);
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    switch (K) {
        case 1: iir_launch_k<S, 1>(in, (long)ld_in, lengths, f, powers, scale, out, (long)ld_out, ws, B, st); break;
        case 2: iir_launch_k<S, 2>(in, (long)ld_in, lengths, f, powers, scale, out, (long)ld_out, ws, B, st); break;
        case 3: iir_launch_k<S, 3>(in, (long)ld_in, lengths, f, powers, scale, out, (long)ld_out, ws, B, st); break;
        default: iir_launch_k<S, 4>(in, (long)ld_in, lengths, f, powers, scale, out, (long)ld_out, ws, B, st); break;
    }
    return efts_check_launch(who);
}

}  // namespace efts

using namespace efts;

extern "C" int64_t efts_iir_workspace_bytes(int32_t B, int64_t max_len) {
    if (B <= 0 || B > 65535 || max_len < 1 || max_len > 0x7fffffffLL - 4 * 2048) return 0;
    return (int64_t)B * iir_nseg(max_len) * IIR_NMAX * 8;
}

extern "C" int efts_iir(const float* in, int64_t ld_in, const int32_t* lengths, const double* sos, int32_t sections, const double* powers, float* out,
                        int64_t ld_out, void* workspace, int32_t B, void* stream) {
    return iir_launch<float>(in, ld_in, lengths, sos, sections, powers, 1.f, out, ld_out, workspace, B, stream, "efts_iir");
}

extern "C" int efts_iir_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, const double* sos, int32_t sections, const double* powers,
                              float pcm_scale, float* out, int64_t ld_out, void* workspace, int32_t B, void* stream) {
    return iir_launch<short>((const short*)in, ld_in, lengths, sos, sections, powers, pcm_scale, out, ld_out, workspace, B, stream, "efts_iir_pcm16");
}
