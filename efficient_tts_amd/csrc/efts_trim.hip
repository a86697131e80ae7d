// efts_trim.hip -- cutting the silence at both ends of a recording and bringing it to one level (include/efts_abi.h has the definition;
// efficient_tts_amd/trim.py is the host side).  Three launches, no host synchronisation, no allocation, no atomics:
//
//   A  trim_energy_kernel : (efts_trim_energy.h, shared with efts_pauses.hip) reads the samples once.  A workgroup stages the samples of `F` consecutive frames ((F - 1) H + W of them) in LDS
//                           -- 16-byte global loads wherever the row's address allows, scalar edges, 0 by predicate outside [0, len) -- and
//                           writes, per frame t, the energy E_t and, per hop chunk c (samples c H .. c H + H - 1), the peak max |x|.
//                           When H divides W (and H >= 64) a frame is W / H hop segments: the segment sums are taken once and W / H of them
//                           are added per frame; neighbouring workgroups overlap by W / H - 1 segments, nothing is read W / H times.
//   B  trim_bounds_kernel : one workgroup per item, on the workspace alone: E_max, the first and last sound frame, the bounds, the peak over
//                           the chunks of [start, end), the gain.  Writes new_len, start, gain.
//   C  trim_copy_kernel   : the compacting, scaling copy.  The source offset `start` is arbitrary: the span is staged in LDS with the same
//                           aligned wide loads as in A and leaves as float4 stores (dword stores when the output row is not 16-byte aligned),
//                           together with the zeros behind new_len.
//
// The staging puts sample i of the span at LDS index sh + i, sh = the row's misalignment in samples, so that the LDS side of every 16-byte
// copy is aligned as well.  Every sum is taken by LOGICAL index in the span, never by address: an item's bits do not depend on where its row lies.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_internal.h"
#include "efts_stft_frame.h"
#include "efts_trim_energy.h"

namespace efts {

// ---- launch B
template <typename S>
__global__ __launch_bounds__(TR_THREADS) void trim_bounds_kernel(const int* __restrict__ lengths, long ld_in, int H, double r, int keep_frames, float peak,
                                                                 float plain_gain, const typename tr_traits<S>::energy_t* __restrict__ energy,
                                                                 const typename tr_traits<S>::peak_t* __restrict__ chunk_peak, int T_max,
                                                                 int* __restrict__ new_len, int* __restrict__ start_out, float* __restrict__ gain) {
    typedef typename tr_traits<S>::energy_t E;
    typedef typename tr_traits<S>::peak_t P;
    __shared__ E s_e[TR_WAVES];
    __shared__ int s_lo[TR_WAVES], s_hi[TR_WAVES];
    __shared__ P s_p[TR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = (int)min((long)max(lengths[b], 0), ld_in);
    const int T = (len + H - 1) / H;
    const E* e = energy + (long)b * T_max;
    E m = 0;
    for (int t = tid; t < T; t += TR_THREADS) { const E v = e[t]; m = v > m ? v : m; }
    m = wave_max_cmp(m);
    if (lane == 0) s_e[wave] = m;
    __syncthreads();
    E e_max = s_e[0];
#pragma unroll
    for (int w = 1; w < TR_WAVES; ++w) e_max = s_e[w] > e_max ? s_e[w] : e_max;
    int start = 0, end = len;
    const bool any = e_max > (E)0;                                 // no sound frame otherwise: an empty or all-zero item
    if (any && keep_frames >= 0) {
        const double dmax = (double)e_max;
        int lo = T, hi = -1;
        for (int t = tid; t < T; t += TR_THREADS)
            if ((double)e[t] * r > dmax) { lo = min(lo, t); hi = max(hi, t); }
        lo = wave_min_cmp(lo);
        hi = wave_max_cmp(hi);
        if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
        __syncthreads();
        lo = s_lo[0], hi = s_hi[0];
#pragma unroll
        for (int w = 1; w < TR_WAVES; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
        // (r > 1: the loudest frame is sound, so lo <= hi here)
        start = (int)max(0L, ((long)lo - keep_frames) * H);
        end = (int)min((long)len, ((long)hi + 1 + keep_frames) * H);
    }
    float g = 1.f;
    if (any) {
        g = plain_gain;
        if (peak > 0.f) {
            const P* cp = chunk_peak + (long)b * T_max;
            P p = 0;
            for (int c = start / H + tid; c < (end + H - 1) / H; c += TR_THREADS) { const P v = cp[c]; p = v > p ? v : p; }
            p = wave_max_cmp(p);
            if (lane == 0) s_p[wave] = p;
            __syncthreads();
            p = s_p[0];
#pragma unroll
            for (int w = 1; w < TR_WAVES; ++w) p = s_p[w] > p ? s_p[w] : p;
            if (p > (P)0) g = __fdiv_rn(peak, (float)p);
        }
    }
    if (tid == 0) {
        new_len[b] = end - start;
        start_out[b] = start;
        gain[b] = g;
    }
}

// ---- launch C
template <typename S, bool VEC>
__global__ __launch_bounds__(TR_THREADS) void trim_copy_kernel(const S* __restrict__ in, long ld_in, const int* __restrict__ lengths,
                                                               const int* __restrict__ new_len, const int* __restrict__ start_in,
                                                               const float* __restrict__ gain, float* __restrict__ out, long ld_out) {
    __shared__ __attribute__((aligned(16))) S xs[TR_COPY + 8];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long o0 = (long)blockIdx.x * TR_COPY;
    const int len = (int)min((long)max(lengths[b], 0), ld_in);
    const int start = min(max(start_in[b], 0), len);
    const int n_new = min(max(new_len[b], 0), len - start);       // (what launch B wrote; clamped so that nothing outside the item can be read)
    const float g = gain[b];
    const int n_row = (int)min((long)TR_COPY, ld_out - o0);                // outputs of this block that exist in the row
    const int n_valid = (int)max(0L, min((long)TR_COPY, (long)n_new - o0));   // ... and that belong to the item
    float* orow = out + (long)b * ld_out + o0;
    int sh = 0;
    if (n_valid > 0) {
        sh = tr_stage(xs, in + (long)b * ld_in, (long)start + o0, n_valid, start + n_new, tid);
        __syncthreads();
    }
    const S* x = xs + sh;
    if (VEC) {                                                     // the row and o0 are 16-byte aligned
        const int n4 = n_row / 4;
        for (int q = tid; q < n4; q += TR_THREADS) {
            const int j = 4 * q;
            float4 v;
            v.x = j + 0 < n_valid ? pcm_sample(x, j + 0, 1.f) * g : 0.f;
            v.y = j + 1 < n_valid ? pcm_sample(x, j + 1, 1.f) * g : 0.f;
            v.z = j + 2 < n_valid ? pcm_sample(x, j + 2, 1.f) * g : 0.f;
            v.w = j + 3 < n_valid ? pcm_sample(x, j + 3, 1.f) * g : 0.f;
            *(float4*)(orow + j) = v;
        }
        for (int j = 4 * n4 + tid; j < n_row; j += TR_THREADS) orow[j] = j < n_valid ? pcm_sample(x, j, 1.f) * g : 0.f;
    } else {
        for (int j = tid; j < n_row; j += TR_THREADS) orow[j] = j < n_valid ? pcm_sample(x, j, 1.f) * g : 0.f;
    }
}

}  // namespace efts

using namespace efts;

extern "C" int64_t efts_trim_workspace_bytes(int32_t B, int64_t max_len, int32_t H, int32_t pcm16) {
    if (B <= 0 || max_len <= 0 || H <= 0) return 0;
    const int64_t T_max = (max_len + H - 1) / H;
    return efts_round16((int64_t)B * T_max * (pcm16 ? 8 : 4)) + efts_round16((int64_t)B * T_max * 4);
}

template <typename S>
static int trim_launch(const S* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t keep_frames, float peak, float plain_gain,
                       float* out, int64_t ld_out, int32_t* new_len, int32_t* start, float* gain, void* workspace, int32_t B, void* stream, const char* who) {
    typedef typename tr_traits<S>::energy_t E;
    typedef typename tr_traits<S>::peak_t P;
    if (B <= 0 || B > 65535) return efts_fail(EFTS_ESHAPE, "%s: 1 .. 65535 items per launch", who);
    if (ld_in <= 0 || ld_in > 0x7fffffffLL - 2 * 2048 || ld_out < ld_in || ld_out > 0x7fffffffLL - TR_COPY)
        return efts_fail(EFTS_ESHAPE, "%s: ld_in must be positive, ld_out >= ld_in, both below 2^31", who);
    if (W != 512 && W != 1024 && W != 2048) return efts_fail(EFTS_ESHAPE, "%s: frame length %d (512, 1024 or 2048)", who, W);
    if (H < 1 || H > W || ((W - H) & 1)) return efts_fail(EFTS_ESHAPE, "%s: hop %d must lie in 1 .. %d with frame length - hop even", who, H, W);
    if (!in || !lengths || !out || !new_len || !start || !gain || !workspace) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (((uintptr_t)in % sizeof(S)) || ((uintptr_t)out & 3) || ((uintptr_t)lengths & 3) || ((uintptr_t)new_len & 3) || ((uintptr_t)start & 3) ||
        ((uintptr_t)gain & 3) || ((uintptr_t)workspace & 15))
        return efts_fail(EFTS_EINVAL, "%s: misaligned pointer (samples and 32-bit arrays to their element, the workspace to 16 bytes)", who);
    if (!(r > 1.0)) return efts_fail(EFTS_EINVAL, "%s: the threshold ratio r = 10^(top_db / 10) must be > 1", who);
    const int T_max = (int)((ld_in + H - 1) / H);
    E* energy = (E*)workspace;
    P* chunk_peak = (P*)((char*)workspace + efts_round16((int64_t)B * T_max * (int64_t)sizeof(E)));
    hipStream_t st = (hipStream_t)stream;
    tr_launch_energy<S, true>(in, ld_in, lengths, W, H, energy, chunk_peak, T_max, B, st);
    hipLaunchKernelGGL(trim_bounds_kernel<S>, dim3((unsigned)B), dim3(TR_THREADS), 0, st, lengths, (long)ld_in, H, r, keep_frames, peak, plain_gain, energy,
                       chunk_peak, T_max, new_len, start, gain);
    const dim3 grid((unsigned)((ld_out + TR_COPY - 1) / TR_COPY), (unsigned)B);
    if (((uintptr_t)out & 15) == 0 && ld_out % 4 == 0)
        hipLaunchKernelGGL((trim_copy_kernel<S, true>), grid, dim3(TR_THREADS), 0, st, in, (long)ld_in, lengths, new_len, start, gain, out, (long)ld_out);
    else
        hipLaunchKernelGGL((trim_copy_kernel<S, false>), grid, dim3(TR_THREADS), 0, st, in, (long)ld_in, lengths, new_len, start, gain, out, (long)ld_out);
    return efts_check_launch(who);
}

extern "C" int efts_trim(const float* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t keep_frames, float peak, float* out,
                         int64_t ld_out, int32_t* new_len, int32_t* start, float* gain, void* workspace, int32_t B, void* stream) {
    return trim_launch<float>(in, ld_in, lengths, W, H, r, keep_frames, peak, 1.f, out, ld_out, new_len, start, gain, workspace, B, stream, "efts_trim");
}

extern "C" int efts_trim_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t keep_frames, float peak,
                               float pcm_scale, float* out, int64_t ld_out, int32_t* new_len, int32_t* start, float* gain, void* workspace, int32_t B,
                               void* stream) {
    return trim_launch<short>((const short*)in, ld_in, lengths, W, H, r, keep_frames, peak, pcm_scale, out, ld_out, new_len, start, gain, workspace, B, stream,
                              "efts_trim_pcm16");
}
