// efts_pauses.hip -- shortening the long pauses inside a recording (include/efts_abi.h has the definition; efficient_tts_amd/pauses.py is the
// host side).  Three launches, no host synchronisation, no allocation, no atomics, no launch geometry from device data:
//
//   A  trim_energy_kernel : the trimmer's frame energies (efts_trim_energy.h), without the chunk peaks.
//   B  pauses_plan_kernel : one workgroup per item, on the workspace alone.  T chunks are walked in tiles of EFTS_PAUSES_TILE, one chunk per
//                           thread, four times; every scan is a wave scan (__shfl_up over 64 lanes), combined across the waves through LDS and
//                           carried from tile to tile in a register that every thread holds:
//                             1  E_max (a reduction);
//                             2  forward: prev[c] = the nearest sound chunk at or in front of c (inclusive max-scan of `sound ? c : -1`);
//                                prev[c] == c says that c is sound, prev[c] == -1 that no sound chunk lies in front of it;
//                             3  backward: next[c] = the nearest sound chunk at or behind c (inclusive min-scan of `sound ? c : T`, the tile
//                                mirrored).  A quiet chunk with prev >= 0 and next < T lies in the pause [prev + 1, next): its position and the
//                                pause's length follow, and so does its code: dropped, kept, or kept as the chunk in front of a joint
//                                (then the code is the sample b that the fade runs into);
//                             4  forward: dst[c] = the exclusive sum of the keep flags; chunk_src[dst] = c, joint[dst] = the code.
//                           A run that crosses a tile boundary is one run: prev and next are global chunk indices, the carry hands them on.
//   C  pauses_copy_kernel : the grid runs over (item, span of output chunks).  An output chunk is read at chunk_src, 16 bytes at a time where
//                           the rows' addresses and H allow; the chunk in front of a joint gets the fade on its last F samples; zeros behind
//                           new_len up to ld_out.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_internal.h"
#include "efts_trim_energy.h"

namespace efts {

constexpr int PA_THREADS = EFTS_PAUSES_TILE, PA_WAVES = PA_THREADS / 64;
constexpr int PA_COPY = 4096;                              // outputs of one workgroup of launch C: max(1, PA_COPY / H) chunks
constexpr int PA_DROP = -2, PA_KEEP = -1;                  // codes of launch B's pass 3; >= 0: kept, and the joint's sample b

// Inclusive scan over the PA_THREADS threads of the workgroup in thread order, `total` = the value of the last thread.  Both barriers
// are inside: s_w can be used again right away.
template <typename OP>
__device__ __forceinline__ int pa_block_scan(int v, OP op, int* s_w, int tid, int& total) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o);
        if (lane >= o) v = op(t, v);
    }
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    int acc = s_w[0];
    if (wave == 0) acc = v;
#pragma unroll
    for (int w = 1; w < PA_WAVES; ++w) {
        if (w == wave) acc = op(acc, v);                   // (acc: waves 0 .. w - 1, then this thread's)
        else if (w < wave) acc = op(acc, s_w[w]);
    }
    total = s_w[0];
#pragma unroll
    for (int w = 1; w < PA_WAVES; ++w) total = op(total, s_w[w]);
    __syncthreads();
    return acc;
}

// ---- launch B
template <typename S>
__global__ __launch_bounds__(PA_THREADS) void pauses_plan_kernel(const int* __restrict__ lengths, long ld_in, int H, double r, int M,
                                                                 const typename tr_traits<S>::energy_t* __restrict__ energy, int* __restrict__ code_ws,
                                                                 int* __restrict__ joint_ws, int T_max, int* __restrict__ chunk_src,
                                                                 int* __restrict__ new_len, int* __restrict__ removed, int* __restrict__ pauses) {
    typedef typename tr_traits<S>::energy_t E;
    __shared__ E s_e[PA_WAVES];
    __shared__ int s_w[PA_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = (int)min((long)max(lengths[b], 0), ld_in);
    const int T = (len + H - 1) / H;
    const E* e = energy + (long)b * T_max;
    int* code = code_ws + (long)b * T_max;
    int* joint = joint_ws + (long)b * T_max;
    int* src = chunk_src + (long)b * T_max;
    const int head = (M + 1) / 2, tail = M / 2;
    // pass 1
    E m = 0;
    for (int t = tid; t < T; t += PA_THREADS) { const E v = e[t]; m = v > m ? v : m; }
    m = wave_max_cmp(m);
    if (lane == 0) s_e[wave] = m;
    __syncthreads();
    E e_max = s_e[0];
#pragma unroll
    for (int w = 1; w < PA_WAVES; ++w) e_max = s_e[w] > e_max ? s_e[w] : e_max;
    const double dmax = (double)e_max;
    // pass 2 (code[] holds prev)
    int carry = -1, total;
    for (int c0 = 0; c0 < T; c0 += PA_THREADS) {
        const int c = c0 + tid;
        const bool sound = c < T && (double)e[c] * r > dmax;       // (E_max == 0: 0 > 0, no frame is sound)
        const int prev = max(carry, pa_block_scan(sound ? c : -1, [](int a, int v) { return max(a, v); }, s_w, tid, total));
        if (c < T) code[c] = prev;
        carry = max(carry, total);
    }
    __syncthreads();                                               // (global writes of this workgroup, read by other threads of it below)
    // pass 3 (code[] from prev to the code), the tiles from the last to the first, thread `tid` on chunk c0 + PA_THREADS - 1 - tid
    carry = T;
    for (int c0 = (T - 1) / PA_THREADS * PA_THREADS; c0 >= 0 && T > 0; c0 -= PA_THREADS) {
        const int c = c0 + PA_THREADS - 1 - tid;
        const int prev = c < T ? code[c] : -1;
        const bool sound = c < T && prev == c;
        const int next = min(carry, pa_block_scan(sound ? c : T, [](int a, int v) { return min(a, v); }, s_w, tid, total));
        if (c < T) {
            int k = PA_KEEP;
            if (!sound && prev >= 0 && next < T) {                 // in the pause [prev + 1, next)
                const int n = next - prev - 1, pos = c - prev - 1;
                if (n > M) {
                    if (pos >= head && pos < n - tail) k = PA_DROP;
                    else if (pos == head - 1) k = (next - tail) * H;      // the joint: < len, since next <= t_last
                }
            }
            code[c] = k;
        }
        carry = min(carry, total);
    }
    __syncthreads();
    // pass 4
    carry = 0;
    int n_joint = 0;
    for (int c0 = 0; c0 < T; c0 += PA_THREADS) {
        const int c = c0 + tid;
        const int k = c < T ? code[c] : PA_DROP;
        const int keep = k != PA_DROP;
        const int dst = carry + pa_block_scan(keep, [](int a, int v) { return a + v; }, s_w, tid, total) - keep;
        if (keep) {
            src[dst] = c;
            joint[dst] = k;
            n_joint += k >= 0;
        }
        carry += total;
    }
    const int kept = carry;                                        // chunks of the output: T - kept were removed, whole chunks all of them
    for (int j = kept + tid; j < T_max; j += PA_THREADS) src[j] = -1;
    n_joint = wave_sum(n_joint);
    if (lane == 0) s_w[wave] = n_joint;
    __syncthreads();
    if (tid == 0) {
        int np = 0;
#pragma unroll
        for (int w = 0; w < PA_WAVES; ++w) np += s_w[w];
        const int rem = (T - kept) * H;
        new_len[b] = len - rem;
        removed[b] = rem;
        pauses[b] = np;
    }
}

// ---- launch C
__device__ __forceinline__ float pa_sample(const float* x, int i, float) { return x[i]; }
__device__ __forceinline__ float pa_sample(const short* x, int i, float scale) { return __fmul_rn((float)x[i], scale); }

// Output sample k of an output chunk that is read at source chunk sc, jb its joint code.  Nothing outside [0, len) is read.
template <typename S>
__device__ __forceinline__ float pa_one(const S* x, int len, int H, int F, const float* __restrict__ fade, int sc, int jb, int k, float scale) {
    const long i = (long)sc * H + k;
    if (sc < 0 || i >= len) return 0.f;
    const float xa = pa_sample(x, (int)i, scale);
    const int kk = k - (H - F);
    if (jb < 0 || kk < 0) return xa;
    const long ib = (long)jb - F + kk;
    if (ib < 0 || ib >= len) return xa;
    const float xb = pa_sample(x, (int)ib, scale);
    return fmaf(fade[kk], __fsub_rn(xb, xa), xa);
}

template <typename S, bool VEC>
__global__ __launch_bounds__(TR_THREADS) void pauses_copy_kernel(const S* __restrict__ in, long ld_in, const int* __restrict__ lengths, int H, int F,
                                                                 const float* __restrict__ fade, float scale, const int* __restrict__ new_len,
                                                                 const int* __restrict__ chunk_src, const int* __restrict__ joint_ws, int T_max, int span,
                                                                 float* __restrict__ out, long ld_out) {
    constexpr int V = tr_traits<S>::V;
    const int b = blockIdx.y, tid = threadIdx.x;
    const long o0 = (long)blockIdx.x * span;
    const int len = (int)min((long)max(lengths[b], 0), ld_in);
    const int n_new = min(max(new_len[b], 0), len);
    const int n_row = (int)min((long)span, ld_out - o0);          // outputs of this block that exist in the row
    const S* x = in + (long)b * ld_in;
    const int* src = chunk_src + (long)b * T_max;
    const int* joint = joint_ws + (long)b * T_max;
    float* orow = out + (long)b * ld_out + o0;
    const int j0 = (int)(o0 / H);                                  // (span is a multiple of H: the block starts on a chunk)
    if (VEC) {                                                     // both rows 16-byte aligned, V | H, 4 | ld_out: a group of V lies in one chunk
        for (int g = tid * V; g < n_row; g += TR_THREADS * V) {
            const long o = o0 + g;
            float v[V];
            if (o >= n_new) {
#pragma unroll
                for (int q = 0; q < V; ++q) v[q] = 0.f;
            } else {
                const int j = j0 + g / H, k = g % H;
                const int sc = src[j], jb = joint[j];
                const long i = (long)sc * H + k;
                if (sc >= 0 && o + V <= n_new && i + V <= len && (jb < 0 || k + V <= H - F)) {
                    const uint4 raw = *(const uint4*)(x + i);
                    if constexpr (sizeof(S) == 4) {
                        v[0] = __uint_as_float(raw.x), v[1] = __uint_as_float(raw.y), v[2] = __uint_as_float(raw.z), v[3] = __uint_as_float(raw.w);
                    } else {
                        const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
                        for (int q = 0; q < V; ++q) v[q] = __fmul_rn((float)(short)(w[(q >> 1) & 3] >> (16 * (q & 1))), scale);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < V; ++q) v[q] = o + q < n_new ? pa_one(x, len, H, F, fade, sc, jb, k + q, scale) : 0.f;
                }
            }
#pragma unroll
            for (int q = 0; q < V; q += 4)
                if (g + q < n_row) *(float4*)(orow + g + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
        }
    } else {
        for (int g = tid; g < n_row; g += TR_THREADS) {
            const long o = o0 + g;
            float v = 0.f;
            if (o < n_new) {
                const int j = j0 + g / H;
                v = pa_one(x, len, H, F, fade, src[j], joint[j], g % H, scale);
            }
            orow[g] = v;
        }
    }
}

}  // namespace efts

using namespace efts;

extern "C" int64_t efts_pauses_workspace_bytes(int32_t B, int64_t max_len, int32_t H, int32_t pcm16) {
    if (B <= 0 || max_len <= 0 || H <= 0) return 0;
    const int64_t T_max = (max_len + H - 1) / H;
    return efts_round16((int64_t)B * T_max * (pcm16 ? 8 : 4)) + 2 * efts_round16((int64_t)B * T_max * 4);
}

template <typename S>
static int pauses_launch(const S* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t M, int32_t F, const float* fade,
                         float scale, float* out, int64_t ld_out, int32_t* new_len, int32_t* removed, int32_t* pauses, int32_t* chunk_src, void* workspace,
                         int32_t B, void* stream, const char* who) {
    typedef typename tr_traits<S>::energy_t E;
    typedef typename tr_traits<S>::peak_t P;
    constexpr int V = tr_traits<S>::V;
    if (B <= 0 || B > 65535) return efts_fail(EFTS_ESHAPE, "%s: 1 .. 65535 items per launch", who);
    if (ld_in <= 0 || ld_in > 0x7fffffffLL - 2 * 2048 || ld_out < ld_in || ld_out > 0x7fffffffLL - PA_COPY)
        return efts_fail(EFTS_ESHAPE, "%s: ld_in must be positive, ld_out >= ld_in, both below 2^31", who);
    if (W != 512 && W != 1024 && W != 2048) return efts_fail(EFTS_ESHAPE, "%s: frame length %d (512, 1024 or 2048)", who, W);
    if (H < 1 || H > W || ((W - H) & 1)) return efts_fail(EFTS_ESHAPE, "%s: hop %d must lie in 1 .. %d with frame length - hop even", who, H, W);
    if (M < 1 || M > (1 << 30)) return efts_fail(EFTS_ESHAPE, "%s: the longest pause kept whole, M = %d chunks, must lie in 1 .. 2^30", who, M);
    if (F < 0 || F > H) return efts_fail(EFTS_ESHAPE, "%s: fade length %d must lie in 0 .. %d, the hop", who, F, H);
    if (!in || !lengths || !out || !new_len || !removed || !pauses || !chunk_src || !workspace || (F > 0 && !fade))
        return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (((uintptr_t)in % sizeof(S)) || ((uintptr_t)out & 3) || ((uintptr_t)lengths & 3) || ((uintptr_t)new_len & 3) || ((uintptr_t)removed & 3) ||
        ((uintptr_t)pauses & 3) || ((uintptr_t)chunk_src & 3) || ((uintptr_t)fade & 3) || ((uintptr_t)workspace & 15))
        return efts_fail(EFTS_EINVAL, "%s: misaligned pointer (samples and 32-bit arrays to their element, the workspace to 16 bytes)", who);
    if (!(r > 1.0)) return efts_fail(EFTS_EINVAL, "%s: the threshold ratio r = 10^(top_db / 10) must be > 1", who);
    const int T_max = (int)((ld_in + H - 1) / H);
    const int64_t words = efts_round16((int64_t)B * T_max * 4);
    E* energy = (E*)workspace;
    int* code = (int*)((char*)workspace + efts_round16((int64_t)B * T_max * (int64_t)sizeof(E)));
    int* joint = (int*)((char*)code + words);
    hipStream_t st = (hipStream_t)stream;
    tr_launch_energy<S, false>(in, ld_in, lengths, W, H, energy, (P*)nullptr, T_max, B, st);
    hipLaunchKernelGGL(pauses_plan_kernel<S>, dim3((unsigned)B), dim3(PA_THREADS), 0, st, lengths, (long)ld_in, H, r, M, energy, code, joint, T_max, chunk_src,
                       new_len, removed, pauses);
    const int span = max(1, PA_COPY / H) * H;
    const dim3 grid((unsigned)((ld_out + span - 1) / span), (unsigned)B);
    const bool vec = ((uintptr_t)in & 15) == 0 && ld_in % V == 0 && H % V == 0 && ((uintptr_t)out & 15) == 0 && ld_out % 4 == 0;
    if (vec)
        hipLaunchKernelGGL((pauses_copy_kernel<S, true>), grid, dim3(TR_THREADS), 0, st, in, (long)ld_in, lengths, H, F, fade, scale, new_len, chunk_src, joint,
                           T_max, span, out, (long)ld_out);
    else
        hipLaunchKernelGGL((pauses_copy_kernel<S, false>), grid, dim3(TR_THREADS), 0, st, in, (long)ld_in, lengths, H, F, fade, scale, new_len, chunk_src, joint,
                           T_max, span, out, (long)ld_out);
    return efts_check_launch(who);
}

extern "C" int efts_pauses(const float* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t M, int32_t F, const float* fade,
                           float* out, int64_t ld_out, int32_t* new_len, int32_t* removed, int32_t* pauses, int32_t* chunk_src, void* workspace, int32_t B,
                           void* stream) {
    return pauses_launch<float>(in, ld_in, lengths, W, H, r, M, F, fade, 1.f, out, ld_out, new_len, removed, pauses, chunk_src, workspace, B, stream,
                                "efts_pauses");
}

extern "C" int efts_pauses_pcm16(const int16_t* in, int64_t ld_in, const int32_t* lengths, int32_t W, int32_t H, double r, int32_t M, int32_t F,
                                 const float* fade, float pcm_scale, float* out, int64_t ld_out, int32_t* new_len, int32_t* removed, int32_t* pauses,
                                 int32_t* chunk_src, void* workspace, int32_t B, void* stream) {
    return pauses_launch<short>((const short*)in, ld_in, lengths, W, H, r, M, F, fade, pcm_scale, out, ld_out, new_len, removed, pauses, chunk_src, workspace,
                                B, stream, "efts_pauses_pcm16");
}
