// efts_resample.hip -- sample-rate conversion between integer rates src and dst by a band-limited windowed-sinc interpolator (Kaiser window),
// in its polyphase form: with g = gcd(src, dst), L = dst / g, M = src / g and a host-built table h[L][K], K = 2 W + 1,
//
//   y[n] = sum over kk = 0 .. K-1 of x[i0 - W + kk] * h[p][kk],   i0 = floor(n M / L),  p = (n M) mod L,   x = 0 outside [0, len)
//
// (efficient_tts_amd/resample.py builds the table; include/efts_abi.h has the definition).  fp32, no atomics, one fixed order of the sum.
//
// One workgroup produces RS_NB consecutive outputs of one item.  The wide arithmetic is done once per workgroup: pos0 = n0 M in 64 bits gives
// the first input sample `base` and the first phase p0; everything inside is a 32-bit offset from them.  The input window of the block
// (base - W .. base + floor((p0 + (RS_NB - 1) M) / L) + W) is staged in LDS as fp32 -- int16 PCM is converted and scaled there -- with every
// sample outside [0, len) produced as 0 by predicate, never read.
//
// Thread mapping: neighbours share a PHASE.  16 lanes work on one output, lane l on kk = l, l + 16, ...: their table reads are 64 contiguous
// bytes of one row (coalesced through L2) and their window reads 16 contiguous LDS words (conflict-free); the 16 partial sums are added by
// a 4-step butterfly.  And the same 16 lanes run the RS_R outputs of the block that share this phase (n, n + L, n + 2 L, ...: their windows
// lie M samples apart) on one table value held in a register, so a table row is read once per RS_R outputs.  A mapping with consecutive n on
// consecutive lanes makes every lane stream its own table row (64 cache lines per load instruction); stores stay coalesced here as well,
// because the results go through an LDS row and leave in order, together with the zeros behind the item's end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_internal.h"
#include "efts_stft_frame.h"

namespace efts {

constexpr int RS_NB = 512, RS_THREADS = 256, RS_LANES = 16, RS_R = 4, RS_GROUPS = RS_THREADS / RS_LANES;
constexpr long RS_TABLE_MAX = 1L << 20;                   // floats: 4 MiB
constexpr int RS_LDS_MAX = 64 * 1024;                     // bytes of window + result row

template <typename SAMPLE>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const SAMPLE* __restrict__ in, long ld_in, const int* __restrict__ lengths,
                                                              const float* __restrict__ table, int L, int M, int W, float* __restrict__ out,
                                                              long ld_out, int* __restrict__ out_lengths, float pcm_scale) {
    extern __shared__ float rs_lds[];                     // [RS_NB] results, then the input window
    float* ys = rs_lds;
    float* xs = rs_lds + RS_NB;
    const int b = blockIdx.y, tid = threadIdx.x, K = 2 * W + 1;
    const int len = (int)min((long)max(lengths[b], 0), ld_in);
    const long out_len = min(((long)len * L + M - 1) / M, ld_out);
    const long n0 = (long)blockIdx.x * RS_NB;
    if (blockIdx.x == 0 && tid == 0) out_lengths[b] = (int)out_len;
    float* orow = out + (long)b * ld_out + n0;
    const int n_row = (int)min((long)RS_NB, ld_out - n0);                 // outputs of this block that exist in the row
    const int n_valid = (int)max(0L, min((long)RS_NB, out_len - n0));     // ... and that belong to the item
    if (n_valid > 0) {
        // ---- once per workgroup, in 64 bits
        const long pos0 = n0 * M;
        const long base = pos0 / L;
        const int p0 = (int)(pos0 - base * L);
        const long lo = base - W;                                          // input sample of xs[0]
        const int span = (p0 + (RS_NB - 1) * M) / L + K;
        const int idx_lo = (int)min((long)span, max(0L, -lo)), idx_hi = (int)max(0L, min((long)span, (long)len - lo));
        const SAMPLE* src = in + (long)b * ld_in + lo;                     // only src[idx_lo .. idx_hi) is read: [0, len) of the item
        for (int i = tid; i < span; i += RS_THREADS) xs[i] = (i >= idx_lo && i < idx_hi) ? pcm_sample(src, i, pcm_scale) : 0.f;
        __syncthreads();
        // ---- work items: (phase class c, chunk q): outputs j = c + L (q RS_R + r), r < RS_R, of this block
        const int Lc = min(L, RS_NB);
        const int Q = ((RS_NB + L - 1) / L + RS_R - 1) / RS_R;
        const int lane = tid & (RS_LANES - 1);
        for (int t = tid / RS_LANES; t < Lc * Q; t += RS_GROUPS) {
            const int q = t / Lc, c = t - q * Lc;
            const int pos = p0 + c * M;
            const int ib = pos / L, p = pos - ib * L;
            const int j0 = c + L * q * RS_R;
            if (j0 >= n_valid) continue;                                   // (uniform over the 16 lanes)
            int xo[RS_R];
#pragma unroll
            for (int r = 0; r < RS_R; ++r) xo[r] = ib + (j0 + r * L < RS_NB ? (q * RS_R + r) * M : 0);
            const float* h = table + (long)p * K;
            float acc[RS_R];
#pragma unroll
            for (int r = 0; r < RS_R; ++r) acc[r] = 0.f;
            for (int kk = lane; kk < K; kk += RS_LANES) {
                const float hv = h[kk];
#pragma unroll
                for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(xs[xo[r] + kk], hv, acc[r]);
            }
#pragma unroll
            for (int r = 0; r < RS_R; ++r) {
#pragma unroll
                for (int o = RS_LANES / 2; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o);
                const int j = j0 + r * L;
                if (lane == 0 && j < n_valid) ys[j] = acc[r];
            }
        }
        __syncthreads();
    }
    for (int j = tid; j < n_row; j += RS_THREADS) orow[j] = j < n_valid ? ys[j] : 0.f;
}

static int rs_gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

}  // namespace efts

using namespace efts;

static int resample_launch(const void* in, bool pcm16, float pcm_scale, int64_t ld_in, const int32_t* lengths, const float* table, int32_t L, int32_t M,
                           int32_t W, float* out, int64_t ld_out, int32_t* out_lengths, int32_t B, void* stream, const char* who) {
    if (!in || !lengths || !table || !out || !out_lengths) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (L <= 0 || M <= 0 || W <= 0 || rs_gcd(L, M) != 1) return efts_fail(EFTS_EINVAL, "%s: L, M, W must be positive, L and M coprime", who);
    if (B <= 0 || B > 65535) return efts_fail(EFTS_ESHAPE, "%s: 1 .. 65535 items per launch", who);
    if (ld_in <= 0 || ld_in > 0x7fffffffLL || ld_out <= 0 || ld_out > 0x7fffffffLL - RS_NB)
        return efts_fail(EFTS_ESHAPE, "%s: ld_in and ld_out must be positive and below 2^31", who);
    const int64_t K = 2 * (int64_t)W + 1;
    if (K * L > RS_TABLE_MAX) return efts_fail(EFTS_ESHAPE, "%s: the table [L][2 W + 1] exceeds 4 MiB", who);
    if ((int64_t)(RS_NB - 1) * M + L > 0x7fffffffLL) return efts_fail(EFTS_ESHAPE, "%s: M too large for 32-bit offsets inside a block", who);
    // the window of one block: floor((p0 + (RS_NB - 1) M) / L) + K samples, p0 < L
    const int64_t span = ((int64_t)(L - 1) + (int64_t)(RS_NB - 1) * M) / L + K;
    const int64_t lds = 4 * (span + RS_NB);
    if (lds > RS_LDS_MAX)
        return efts_fail(EFTS_ESHAPE, "%s: the input window of %d outputs (%lld samples) does not fit %d KiB of LDS: the rate ratio is too steep for one pass",
                         who, RS_NB, (long long)span, RS_LDS_MAX / 1024);
    const dim3 grid((unsigned)((ld_out + RS_NB - 1) / RS_NB), (unsigned)B);
    if (pcm16)
        hipLaunchKernelGGL(resample_kernel<short>, grid, dim3(RS_THREADS), (size_t)lds, (hipStream_t)stream, (const short*)in, (long)ld_in, lengths, table, L, M,
                           W, out, (long)ld_out, out_lengths, pcm_scale);
    else
        hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(RS_THREADS), (size_t)lds, (hipStream_t)stream, (const float*)in, (long)ld_in, lengths, table, L, M,
                           W, out, (long)ld_out, out_lengths, 1.f);
    return efts_check_launch(who);
}

extern "C" int efts_resample(const float* in, int64_t ld_in, const int32_t* lengths, const float* table, int32_t L, int32_t M, int32_t W, float* out,
                             int64_t ld_out, int32_t* out_lengths, int32_t B, void* stream) {
    return resample_launch(in, false, 1.f, ld_in, lengths, table, L, M, W, out, ld_out, out_lengths, B, stream, "efts_resample");
}

extern "C" int efts_resample_pcm16(const int16_t* in, int64_t ld_in, float pcm_scale, const int32_t* lengths, const float* table, int32_t L, int32_t M,
                                   int32_t W, float* out, int64_t ld_out, int32_t* out_lengths, int32_t B, void* stream) {
    return resample_launch(in, true, pcm_scale, ld_in, lengths, table, L, M, W, out, ld_out, out_lengths, B, stream, "efts_resample_pcm16");
}
