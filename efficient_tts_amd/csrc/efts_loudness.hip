// efts_loudness.hip -- integrated loudness after ITU-R BS.1770 / EBU R 128 of a padded batch, and the gain that brings every item to a target
// (include/efts_abi.h has the definition; efficient_tts_amd/loudness.py is the host side).  Three launches, no host synchronisation, no
// allocation, no atomics:
//
//   A  loud_filter_kernel : one THREAD per segment of LD_SEG samples.  The K-weighting filter is a recurrence along time; a thread runs it from
//                           zero state over the 2 h samples in front of its segment (the warm-up: 0.2 s, after which what the 38 Hz high-pass
//                           still remembers of earlier input is below 1e-13 of the output) and then over the segment, where it adds y^2 into the
//                           (at most two) 100 ms sub-blocks that the segment touches and takes max |x|.  The segment at sample 0 needs no
//                           warm-up: x = 0 in front of the item IS the zero state.  Everything on the recurrence is fp64; the launch is bound
//                           by the latency of that dependent chain (two fma per biquad and sample), not by bytes.
//   B  loud_decide_kernel : one workgroup per item, on the workspace alone: the sub-block sums, the 400 ms block powers, the two gates, the
//                           loudness, the peak, the gain.
//   C  loud_scale_kernel  : out = (float) x * gain, zeros behind the length (not launched when only the measurement is asked for).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "efts_internal.h"

namespace efts {

constexpr int LD_SEG = EFTS_LOUDNESS_SEGMENT;              // samples of one thread of launch A
static_assert(LD_SEG <= 800, "a segment may touch at most two sub-blocks: h >= 800 at 8000 Hz");
constexpr int LD_FILTER_THREADS = 64, LD_THREADS = 256, LD_WAVES = LD_THREADS / 64;
constexpr int LD_COPY = 4096;                              // outputs of one workgroup of launch C

struct loud_coef { double sb0, sb1, sb2, sa1, sa2, hb0, hb1, hb2, ha1, ha2; };

__device__ __forceinline__ double ld_sample(const float* row, long i, double) { return (double)row[i]; }
__device__ __forceinline__ double ld_sample(const short* row, long i, double scale) { return (double)row[i] * scale; }
__device__ __forceinline__ float ld_mag(float v) { return fabsf(v); }
__device__ __forceinline__ float ld_mag(short v) { return fabsf((float)v); }      // (exact: |v| <= 32768)

// one sample through both biquads, transposed direct form II, in the order that the header states
struct loud_state {
    double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0;
    __device__ __forceinline__ double step(const loud_coef& c, double x) {
        const double v = fma(c.sb0, x, s1);
        s1 = fma(-c.sa1, v, fma(c.sb1, x, s2));
        s2 = fma(-c.sa2, v, c.sb2 * x);
        const double y = fma(c.hb0, v, t1);
        t1 = fma(-c.ha1, y, fma(c.hb1, v, t2));
        t2 = fma(-c.ha2, y, c.hb2 * v);
        return y;
    }
};

// ---- launch A
template <typename S>
__global__ __launch_bounds__(LD_FILTER_THREADS) void loud_filter_kernel(const S* __restrict__ in, long ld_in, const int* __restrict__ lengths, int h,
                                                                        loud_coef c, double scale, double* __restrict__ part,
                                                                        float* __restrict__ seg_peak, long nseg_max) {
    const int b = blockIdx.y;
    const long s = (long)blockIdx.x * LD_FILTER_THREADS + threadIdx.x;
    const long len = min((long)max(lengths[b], 0), ld_in);
    const long i0 = s * LD_SEG;
    if (i0 >= len) return;                                         // no sample of the item in this segment: nothing of it is read later
    const long i1 = min(len, i0 + LD_SEG);
    const S* row = in + (long)b * ld_in;
    loud_state f;
    for (long i = max(0L, i0 - 2L * h); i < i0; ++i) f.step(c, ld_sample(row, i, scale));
    const long edge = (i0 / h + 1) * h;                            // the first sample of the next sub-block
    double acc0 = 0.0, acc1 = 0.0;
    float pk = 0.f;
    const long m = min(i1, edge);
    for (long i = i0; i < m; ++i) {
        const double y = f.step(c, ld_sample(row, i, scale));
        acc0 = fma(y, y, acc0);
        pk = fmaxf(pk, ld_mag(row[i]));
    }
    for (long i = m; i < i1; ++i) {
        const double y = f.step(c, ld_sample(row, i, scale));
        acc1 = fma(y, y, acc1);
        pk = fmaxf(pk, ld_mag(row[i]));
    }
    double* p = part + ((long)b * nseg_max + s) * 2;
    p[0] = acc0;
    p[1] = acc1;
    seg_peak[(long)b * nseg_max + s] = pk;
}

// the documented order of a workgroup's sum: inside a wave v = v + (the value 32, 16, 8, 4, 2, 1 lanes across), then wave 0 + 1 + 2 + 3
__device__ __forceinline__ double ld_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    __syncthreads();                                               // (sh may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
__device__ __forceinline__ int ld_block_sum(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// ---- launch B
__global__ __launch_bounds__(LD_THREADS) void loud_decide_kernel(const int* __restrict__ lengths, long ld_in, int h, const double* __restrict__ part,
                                                                 const float* __restrict__ seg_peak, long nseg_max, double* __restrict__ sub,
                                                                 long nsub_max, double gamma_a, double target, double ceiling, double scale,
                                                                 double* __restrict__ loudness, float* __restrict__ gain, int* __restrict__ flags,
                                                                 int* __restrict__ blocks) {
    __shared__ double sh_d[LD_WAVES];
    __shared__ int sh_i[LD_WAVES];
    __shared__ float sh_p[LD_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long len = min((long)max(lengths[b], 0), ld_in);
    const long nsub = len / h, nblk = nsub >= 4 ? nsub - 3 : 0, nseg = (len + LD_SEG - 1) / LD_SEG;
    const double* pt = part + (long)b * nseg_max * 2;
    double* sb = sub + (long)b * nsub_max;
    // sub-block k = samples k h .. k h + h - 1: the parts of its segments, first segment first
    for (long k = tid; k < nsub; k += LD_THREADS) {
        const long s_lo = (k * h) / LD_SEG, s_hi = ((k + 1) * h - 1) / LD_SEG;
        double acc = 0.0;
        for (long s = s_lo; s <= s_hi; ++s) acc = acc + pt[2 * s + (k - (s * LD_SEG) / h)];
        sb[k] = acc;
    }
    float pk = 0.f;
    for (long s = tid; s < nseg; s += LD_THREADS) pk = fmaxf(pk, seg_peak[(long)b * nseg_max + s]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));
    if ((tid & 63) == 0) sh_p[tid >> 6] = pk;
    __syncthreads();                                               // sb[] and sh_p[] are written
    pk = fmaxf(fmaxf(sh_p[0], sh_p[1]), fmaxf(sh_p[2], sh_p[3]));
    const double inv = 1.0 / (4.0 * (double)h);
    // the absolute gate
    double sum = 0.0;
    int cnt = 0;
    for (long j = tid; j < nblk; j += LD_THREADS) {
        const double z = (((sb[j] + sb[j + 1]) + sb[j + 2]) + sb[j + 3]) * inv;
        if (z > gamma_a) { sum = sum + z; ++cnt; }
    }
    const double sum_a = ld_block_sum(sum, sh_d);
    const int n_a = ld_block_sum(cnt, sh_i);
    // the relative gate
    const double gamma_r = n_a > 0 ? 0.1 * (sum_a / (double)n_a) : 0.0;
    sum = 0.0;
    cnt = 0;
    for (long j = tid; j < nblk; j += LD_THREADS) {
        const double z = (((sb[j] + sb[j + 1]) + sb[j + 2]) + sb[j + 3]) * inv;
        if (z > gamma_a && z > gamma_r) { sum = sum + z; ++cnt; }
    }
    const double sum_g = ld_block_sum(sum, sh_d);
    const int n_g = ld_block_sum(cnt, sh_i);
    if (tid != 0) return;
    int fl = 0;
    double L = -INFINITY;
    float gf = (float)scale;                                       // gain 1
    if (n_a > 0 && n_g > 0) {
        L = -0.691 + 10.0 * log10(sum_g / (double)n_g);
        const double g = pow(10.0, (target - L) / 20.0);
        const double p = (double)pk * scale;
        if (ceiling > 0.0 && g * p > ceiling) {
            fl |= 2;
            gf = __double2float_rd((ceiling / p) * scale);
            for (int it = 0; it < 4 && (double)__fmul_rn(pk, gf) > ceiling; ++it) gf = nextafterf(gf, 0.f);
        } else {
            gf = (float)(g * scale);
        }
    } else {
        fl |= 1;
    }
    loudness[b] = L;
    gain[b] = gf;
    flags[b] = fl;
    blocks[2 * b] = n_a;
    blocks[2 * b + 1] = (n_a > 0 && n_g > 0) ? n_g : 0;
}

// ---- launch C
template <typename S, bool VEC>
__global__ __launch_bounds__(LD_THREADS) void loud_scale_kernel(const S* __restrict__ in, long ld_in, const int* __restrict__ lengths,
                                                                const float* __restrict__ gain, float* __restrict__ out, long ld_out) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const long o0 = (long)blockIdx.x * LD_COPY;
    const long len = min((long)max(lengths[b], 0), ld_in);
    const float g = gain[b];
    const S* x = in + (long)b * ld_in;
    float* orow = out + (long)b * ld_out;
    const long o1 = min(ld_out, o0 + LD_COPY);
    if (VEC) {                                                     // the row and o0 are 16-byte aligned, ld_out % 4 == 0
        for (long j = o0 + 4 * tid; j < o1; j += 4 * LD_THREADS) {
            float4 v;
            v.x = j + 0 < len ? (float)x[j + 0] * g : 0.f;
            v.y = j + 1 < len ? (float)x[j + 1] * g : 0.f;
            v.z = j + 2 < len ? (float)x[j + 2] * g : 0.f;
            v.w = j + 3 < len ? (float)x[j + 3] * g : 0.f;
            *(float4*)(orow + j) = v;
        }
    } else {
        for (long j = o0 + tid; j < o1; j += LD_THREADS) orow[j] = j < len ? (float)x[j] * g : 0.f;
    }
}

static inline int64_t ld_nseg(int64_t max_len) { return (max_len + LD_SEG - 1) / LD_SEG; }
static inline bool ld_rate_ok(int32_t fs) { return fs >= 8000 && fs <= 48000 && fs % 10 == 0; }

}  // namespace efts

using namespace efts;

extern "C" int64_t efts_loudness_workspace_bytes(int32_t B, int64_t max_len, int32_t fs) {
    if (B <= 0 || max_len <= 0 || !ld_rate_ok(fs)) return 0;
    const int64_t nseg = ld_nseg(max_len), nsub = max_len / (fs / 10) + 1;
    return efts_round16((int64_t)B * nseg * 16) + efts_round16((int64_t)B * nseg * 4) + efts_round16((int64_t)B * nsub * 8);
}

template <typename S>
static int loudness_launch(const S* in, int64_t ld_in, const int32_t* lengths, int32_t fs, const double* kweight, double target_lufs, double peak_ceiling,
                           double scale, float* out, int64_t ld_out, double* loudness, float* gain, int32_t* flags, int32_t* blocks, void* workspace, int32_t B,
                           void* stream, const char* who) {
    if (B <= 0 || B > 65535) return efts_fail(EFTS_ESHAPE, "%s: 1 .. 65535 items per launch", who);
    if (ld_in <= 0 || ld_in > 0x7fffffffLL - LD_COPY || (out && (ld_out < ld_in || ld_out > 0x7fffffffLL - LD_COPY)))
        return efts_fail(EFTS_ESHAPE, "%s: ld_in must be positive, ld_out >= ld_in, both below 2^31", who);
    if (!ld_rate_ok(fs)) return efts_fail(EFTS_ESHAPE, "%s: sampling rate %d (8000 .. 48000 Hz, a multiple of 10)", who, fs);
    if (!in || !lengths || !kweight || !loudness || !gain || !flags || !blocks || !workspace) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (((uintptr_t)in % sizeof(S)) || ((uintptr_t)out & 3) || ((uintptr_t)lengths & 3) || ((uintptr_t)loudness & 7) || ((uintptr_t)gain & 3) ||
        ((uintptr_t)flags & 3) || ((uintptr_t)blocks & 3) || ((uintptr_t)kweight & 7) || ((uintptr_t)workspace & 15))
        return efts_fail(EFTS_EINVAL, "%s: misaligned pointer (every array to its element, the workspace to 16 bytes)", who);
    if (!std::isfinite(target_lufs) || std::isnan(peak_ceiling) || !std::isfinite(scale) || !(scale > 0.0))
        return efts_fail(EFTS_EINVAL, "%s: the target must be finite, the ceiling a number and pcm_scale > 0", who);
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(kweight[i])) return efts_fail(EFTS_EINVAL, "%s: K-weighting coefficient %d is not finite", who, i);
    const loud_coef c = {kweight[0], kweight[1], kweight[2], kweight[3], kweight[4], kweight[5], kweight[6], kweight[7], kweight[8], kweight[9]};
    const int h = fs / 10;
    const long nseg = (long)ld_nseg(ld_in), nsub = (long)(ld_in / h + 1);
    double* part = (double*)workspace;
    float* seg_peak = (float*)((char*)workspace + efts_round16((int64_t)B * nseg * 16));
    double* sub = (double*)((char*)seg_peak + efts_round16((int64_t)B * nseg * 4));
    const double gamma_a = std::pow(10.0, (-70.0 + 0.691) / 10.0);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(loud_filter_kernel<S>, dim3((unsigned)((nseg + LD_FILTER_THREADS - 1) / LD_FILTER_THREADS), (unsigned)B), dim3(LD_FILTER_THREADS), 0, st,
                       in, (long)ld_in, lengths, h, c, scale, part, seg_peak, nseg);
    hipLaunchKernelGGL(loud_decide_kernel, dim3((unsigned)B), dim3(LD_THREADS), 0, st, lengths, (long)ld_in, h, part, seg_peak, nseg, sub, nsub, gamma_a,
                       target_lufs, peak_ceiling, scale, loudness, gain, flags, blocks);
    if (out) {
        const dim3 grid((unsigned)((ld_out + LD_COPY - 1) / LD_COPY), (unsigned)B);
        if (((uintptr_t)out & 15) == 0 && ld_out % 4 == 0)
            hipLaunchKernelGGL((loud_scale_kernel<S, true>), grid, dim3(LD_THREADS), 0, st, in, (long)ld_in, lengths, gain, out, (long)ld_out);
        else
            hipLaunchKernelGGL((loud_scale_kernel<S, false>), grid, dim3(LD_THREADS), 0, st, in, (long)ld_in, lengths, gain, out, (long)ld_out);
    }
    return efts_check_launch(who);
}

extern "C" int efts_loudness(const float* in, int64_t ld_in, const int32_t* lengths, int32_t fs, const double* kweight, double target_lufs,
                             double peak_ceiling, float* out, int64_t ld_out, double* loudness, float* gain, int32_t* flags, int32_t* blocks,
                             void* workspace, int32_t B, void* stream) {
    return loudness_launch<float>(in, ld_in, lengths, fs, kweight, target_lufs, peak_ceiling, 1.0, out, ld_out, loudness, gain, flags, blocks, workspace, B,
                                  stream, "efts_loudness");
}

extern "C" int efts_loudness_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, int32_t fs, const double* kweight, double target_lufs,
                                   double peak_ceiling, float pcm_scale, float* out, int64_t ld_out, double* loudness, float* gain, int32_t* flags,
                                   int32_t* blocks, void* workspace, int32_t B, void* stream) {
    return loudness_launch<short>((const short*)in, ld_in, lengths, fs, kweight, target_lufs, peak_ceiling, (double)pcm_scale, out, ld_out, loudness, gain,
                                  flags, blocks, workspace, B, stream, "efts_loudness_pcm16");
}
