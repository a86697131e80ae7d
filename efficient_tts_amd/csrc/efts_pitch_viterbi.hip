// efts_pitch_viterbi.hip -- the cheapest path over the per-frame lag candidates of the pitch tracker: efts_f0_viterbi and
// efts_f0_viterbi_workspace_bytes.  include/efts_abi.h has the definition (integer costs in Q16, an integer-only recurrence, one tie rule);
// efficient_tts_amd/pitch.py owns the calls.  No atomics, no floating point in the recurrence: an item gives the same bits alone, in any batch
// position and in any run.
//
// Shape.  One workgroup per item, sequential over the item's frames, one barrier per frame.  Thread s < S owns the voiced state s (lag
// k = tau_min + s, S <= 1022 states fit one workgroup of up to 1024 threads); its lg[k] and its octave term live in registers, so no table is
// staged.  The unvoiced state has only two kinds of predecessor -- itself, and the cheapest voiced state plus vuv_q -- so every thread carries
// its cost in a register (the same value everywhere) and nobody owns it.
//
// Per frame a thread loads and quantises its d' (one coalesced row read per workgroup), takes the minimum over the predecessors, stores its
// back-pointer (uint16, coalesced) and publishes its new cost for the next frame.  What is published is double-buffered in LDS:
//   * per wave, the (cost, state) minimum of its voiced states as one 64-bit key, cost in the high bits: the minimum over the keys is the
//     cheapest voiced state with the lowest index.  After the barrier every thread folds the <= 16 keys itself.
//   * per wave, the COMPACTED list of its states that can still matter (below), in ascending state order: {cost, lg[k]} and the state.
// Costs stay small: frame t stores C(t, s) minus the minimum of frame t - 1, which shifts a whole frame by one constant and leaves every
// argmin where it was.  By induction a stored cost lies in (-2^25, 2^25), for any number of frames.
//
// Pruning, and why it is exact.  Let U = C(t-1, unvoiced) + vuv_q: what reaching a voiced state through the unvoiced state costs.  A voiced
// predecessor p with C(t-1, p) > U gives C(t-1, p) + trans(p, s) >= C(t-1, p) > U for EVERY voiced target s, because trans >= 0: it is
// strictly beaten by the unvoiced predecessor, so it is neither the minimum nor tied with it, and the tie rule never sees it.  For the unvoiced
// target only the cheapest voiced state counts, and the wave keys hold it whether or not it is listed.  So the list of frame t - 1 keeps
// exactly the states with C(t-1, p) <= U -- U is known when the list is written, since the unvoiced cost is a register of every thread --
// and the inner loop runs over the lists of all waves in ascending state order, replacing on strictly smaller only (lowest index wins a tie),
// with the unvoiced predecessor tried last.  On speech the lists hold the lags near the period and its multiples, a small share of S; with
// vuv_q or unvoiced_q so large that nothing can be pruned the loop is the full S^2 and just as exact.
//
// Back-trace, in the same launch: the record is read back through LDS in chunks of whole frames, one thread walks a chunk, then one wave per
// frame writes lag, f0 (efts_yin's parabola at the path's lag) and the aperiodicity.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "efts_internal.h"

namespace efts {

constexpr int VIT_Q = 65536;
constexpr int VIT_MAX_THREADS = 1024, VIT_MAX_WAVES = VIT_MAX_THREADS / 64;
constexpr int VIT_BT_ENTRIES = 12288, VIT_BT_ROWS = 256;       // back-pointers of one chunk in LDS (24 KiB); most frames per chunk
constexpr int VIT_PAD_COST = 0x3fffffff;                         // a list's padding: above every cost, and no overflow with a transition on top
constexpr long long VIT_KEY_MAX = 0x7fffffffffffffffLL;

struct vit_args {
    const float* cmnd; long item_stride, frame_stride;
    const int* frames; const int* lg;
    float* f0; float* aper; int* lag;
    unsigned short* ws; long ws_item;      // back-pointers, entries per item
    int T, tau_min, tau_max;
    float sr;
    int unvoiced_q, octave_q, jump_q, vuv_q;
};

// q(x) of the header: NaN and everything from 4 up land on 4 Q, everything down to -inf on -4 Q (d' itself is never negative)
__device__ __forceinline__ int vit_quant(float x) { return x < 4.f ? (x > -4.f ? (int)rintf(x * 65536.f) : -4 * VIT_Q) : 4 * VIT_Q; }

// (jump_q |a - b|) >> 16: both factors are below 2^24 (jump_q <= 16 Q = 2^20, lg <= 10 Q), the masks let the 24-bit multipliers take it
__device__ __forceinline__ int vit_trans(int jump_q, int a, int b) {
    const unsigned d = (unsigned)abs(a - b) & 0xffffffu;
    return (int)(((unsigned long long)d * (unsigned long long)((unsigned)jump_q & 0xffffffu)) >> 16);
}

__device__ __forceinline__ long long vit_key_min(long long a, long long b) { return b < a ? b : a; }

__global__ __launch_bounds__(VIT_MAX_THREADS) void viterbi_kernel(vit_args a) {
    __shared__ __attribute__((aligned(16))) int2 cand[2][VIT_MAX_THREADS];                 // {cost, lg[k]} of the listed states, wave w's list at [64 w ..)
    __shared__ unsigned short cand_state[2][VIT_MAX_THREADS];
    __shared__ int cand_count[2][VIT_MAX_WAVES];
    __shared__ long long wave_key[2][VIT_MAX_WAVES];          // (cost << 16 | state) minimum of a wave's voiced states
    __shared__ unsigned short bt[VIT_BT_ENTRIES];
    __shared__ unsigned short path_chunk[VIT_BT_ROWS + 1];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int S = a.tau_max - a.tau_min, S1 = S + 1, T = a.T;
    const int n = max(0, min(a.frames[b], T));                // (uniform over the workgroup)
    float* f0 = a.f0 + (long)b * T;
    float* aper = a.aper + (long)b * T;
    int* lag = a.lag + (long)b * T;
    for (int t = n + tid; t < T; t += blockDim.x) { f0[t] = 0.f; aper[t] = 0.f; lag[t] = 0; }
    if (n == 0) return;                                       // before any barrier

    const bool voiced = tid < S;
    const int k = a.tau_min + tid;
    const int lgk = voiced ? a.lg[k] : 0;
    const int octave = voiced ? (int)(((long long)a.octave_q * (long long)(lgk - a.lg[a.tau_min])) >> 16) : 0;
    const float* item = a.cmnd + (long)b * a.item_stride;
    unsigned short* bp = a.ws + (long)b * a.ws_item;
    if (tid >= nw && tid < VIT_MAX_WAVES) wave_key[0][tid] = wave_key[1][tid] = VIT_KEY_MAX;     // the slots no wave writes

    // the loads above land here, once: otherwise the compiler, which cannot tell the first frame from the others, waits in the inner loop for
    // everything in flight -- the frame's d' and the back-pointer store of the frame before -- on every frame
    __builtin_amdgcn_s_waitcnt(0x0f70);                       // vmcnt(0)
    int du = a.unvoiced_q;                                    // C(t, unvoiced) as stored, the same in every thread
    for (int t = 0; t < n; ++t) {
        const int nxt = t & 1, prv = nxt ^ 1;
        const float x = voiced ? item[(long)t * a.frame_stride + k] : 0.f;
        int mine = 0, obs = 0;
        if (t == 0) obs = vit_quant(x) + octave;
        if (t > 0) {
            long long key = wave_key[prv][lane & (VIT_MAX_WAVES - 1)];
#pragma unroll
            for (int o = VIT_MAX_WAVES / 2; o > 0; o >>= 1) key = vit_key_min(key, __shfl_xor(key, o));
            const int mv = (int)(key >> 16), pv = (int)(key & 0xffff);       // the cheapest voiced state of frame t - 1, lowest index
            const int m = min(mv, du);                                       // frame t - 1's minimum
            const int through_unvoiced = du + a.vuv_q;
            int best = 0x7fffffff, best_at = 0;
            for (int w = 0; w < nw; ++w) {
                const int c = __builtin_amdgcn_readfirstlane(cand_count[prv][w]);
                const int4* e = (const int4*)&cand[prv][w * 64];
                for (int j = 0; j < c; j += 4) {                             // lists are padded to a multiple of four entries
                    const int4 v0 = e[j / 2], v1 = e[j / 2 + 1];             // (broadcasts: every lane reads the same entries)
                    const int c0 = v0.x + vit_trans(a.jump_q, lgk, v0.y), c1 = v0.z + vit_trans(a.jump_q, lgk, v0.w);
                    const int c2 = v1.x + vit_trans(a.jump_q, lgk, v1.y), c3 = v1.z + vit_trans(a.jump_q, lgk, v1.w);
                    if (c0 < best) { best = c0; best_at = w * 64 + j; }
                    if (c1 < best) { best = c1; best_at = w * 64 + j + 1; }
                    if (c2 < best) { best = c2; best_at = w * 64 + j + 2; }
                    if (c3 < best) { best = c3; best_at = w * 64 + j + 3; }
                }
            }
            int pred = S;
            if (through_unvoiced < best) best = through_unvoiced;
            else pred = cand_state[prv][best_at];
            mine = best - m;
            obs = vit_quant(x) + octave;                                     // (the wait for x stands in front of this frame's stores, not behind them)
            if (voiced) bp[(long)t * S1 + tid] = (unsigned short)pred;
            const int through_voiced = mv + a.vuv_q;
            if (tid == 0) bp[(long)t * S1 + S] = (unsigned short)(through_voiced <= du ? pv : S);
            du = a.unvoiced_q + (min(du, through_voiced) - m);
        }
        mine += obs;
        // publish frame t
        const bool listed = voiced && mine <= du + a.vuv_q;
        const unsigned long long mask = __ballot(listed);
        const int listed_n = __popcll(mask);
        if (listed) {
            const int at = wave * 64 + __popcll(mask & ((1ull << lane) - 1ull));
            cand[nxt][at] = make_int2(mine, lgk);
            cand_state[nxt][at] = (unsigned short)tid;
        }
        if (lane < ((4 - (listed_n & 3)) & 3)) cand[nxt][wave * 64 + listed_n + lane] = make_int2(VIT_PAD_COST, 0);      // never the minimum
        long long key = voiced ? (long long)mine * 65536LL + tid : VIT_KEY_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = vit_key_min(key, __shfl_xor(key, o));
        if (lane == 0) { cand_count[nxt][wave] = listed_n; wave_key[nxt][wave] = key; }
        __syncthreads();
    }

    // the final state: the lowest index among the minima of the last frame (the unvoiced state has the highest index)
    long long key = wave_key[(n - 1) & 1][lane & (VIT_MAX_WAVES - 1)];
#pragma unroll
    for (int o = VIT_MAX_WAVES / 2; o > 0; o >>= 1) key = vit_key_min(key, __shfl_xor(key, o));
    int cur = (int)(key >> 16) <= du ? (int)(key & 0xffff) : S;          // thread 0 walks; the state of frame `top`

    const int rows = min(VIT_BT_ROWS, VIT_BT_ENTRIES / S1);
    int top = n - 1;
    for (;;) {                                                // (n alone decides the trip count)
        const int lo = max(0, top - rows);
        const unsigned short* src = bp + (long)(lo + 1) * S1; // the records of frames lo + 1 .. top
        const int count = (top - lo) * S1;
        for (int i = tid; i < count; i += blockDim.x) bt[i] = src[i];
        __syncthreads();
        if (tid == 0) {
            path_chunk[top - lo] = (unsigned short)cur;
            for (int t = top; t > lo; --t) {
                cur = bt[(t - lo - 1) * S1 + cur];
                path_chunk[t - 1 - lo] = (unsigned short)cur;
            }
        }
        __syncthreads();
        // frames lo + 1 .. top (and frame 0 with the last chunk): one wave per frame
        for (int t = (lo == 0 ? 0 : lo + 1) + wave; t <= top; t += nw) {
            const int st = path_chunk[t - lo];
            const float* row = item + (long)t * a.frame_stride;
            if (st < S) {
                if (lane == 0) {
                    const int kk = a.tau_min + st;
                    const float s0 = row[kk - 1], s1 = row[kk], s2 = row[kk + 1];
                    const float den = (s0 - s1) + (s2 - s1);
                    float shift = den == 0.f ? 0.f : 0.5f * (s0 - s2) / den;
                    shift = fminf(1.f, fmaxf(-1.f, shift));
                    f0[t] = a.sr / ((float)kk + shift);
                    aper[t] = s1;
                    lag[t] = kk;
                }
            } else {
                float lowest = __builtin_inff();
                for (int kk = a.tau_min + lane; kk < a.tau_max; kk += 64) lowest = fminf(lowest, row[kk]);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) lowest = fminf(lowest, __shfl_xor(lowest, o));
                if (lane == 0) { f0[t] = 0.f; aper[t] = lowest; lag[t] = 0; }
            }
        }
        if (lo == 0) break;
        top = lo;
    }
}

}  // namespace efts

using namespace efts;

extern "C" int64_t efts_f0_viterbi_workspace_bytes(int32_t T, int32_t tau_min, int32_t tau_max) {
    if (T < 1 || T > EFTS_VITERBI_MAX_FRAMES || tau_min < 2 || !(tau_min < tau_max - 1) || tau_max > EFTS_VITERBI_MAX_LAG) return 0;
    const int64_t bytes = (int64_t)T * (tau_max - tau_min + 1) * 2;
    return (bytes + 15) / 16 * 16;
}

extern "C" int efts_f0_viterbi(const float* cmnd, int64_t item_stride, int64_t frame_stride, const int32_t* frames, const int32_t* lg, float* f0,
                               float* aperiodicity, int32_t* lag, void* workspace, int64_t workspace_bytes, int32_t B, int32_t T, int32_t tau_min,
                               int32_t tau_max, int32_t sampling_rate, int32_t unvoiced_q, int32_t octave_q, int32_t jump_q, int32_t vuv_q,
                               void* stream) {
    const char* who = "efts_f0_viterbi";
    if (!cmnd || !frames || !lg || !f0 || !aperiodicity || !lag || !workspace) return efts_fail(EFTS_EINVAL, "%s: null pointer", who);
    if (tau_min < 2 || !(tau_min < tau_max - 1) || tau_max > EFTS_VITERBI_MAX_LAG)
        return efts_fail(EFTS_ESHAPE, "%s: need 2 <= tau_min < tau_max - 1 and tau_max <= %d (got %d, %d)", who, EFTS_VITERBI_MAX_LAG, tau_min, tau_max);
    if (B < 1 || B > 65535 || T < 1 || T > EFTS_VITERBI_MAX_FRAMES || sampling_rate < 1)
        return efts_fail(EFTS_ESHAPE, "%s: 1 .. 65535 items, T 1 .. %d, sampling_rate >= 1", who, EFTS_VITERBI_MAX_FRAMES);
    if (frame_stride < (int64_t)tau_max + 1 || item_stride < 0)
        return efts_fail(EFTS_ESHAPE, "%s: frame_stride >= tau_max + 1 and item_stride >= 0 (got %lld, %lld)", who, (long long)frame_stride, (long long)item_stride);
    const int32_t costs[4] = {unvoiced_q, octave_q, jump_q, vuv_q};
    for (int i = 0; i < 4; ++i)
        if (costs[i] < 0 || costs[i] > 16 * VIT_Q) return efts_fail(EFTS_ESHAPE, "%s: every cost must lie in 0 .. 16 (Q16: 0 .. %d), got %d", who, 16 * VIT_Q, costs[i]);
    const int64_t per_item = efts_f0_viterbi_workspace_bytes(T, tau_min, tau_max);
    if (workspace_bytes < per_item * B)
        return efts_fail(EFTS_ESHAPE, "%s: workspace of %lld bytes, %d items of %d frames need %lld", who, (long long)workspace_bytes, B, T, (long long)(per_item * B));
    if ((uintptr_t)workspace & 15) return efts_fail(EFTS_EALIGN, "%s: workspace must be 16-byte aligned", who);
    vit_args a;
    a.cmnd = cmnd; a.item_stride = (long)item_stride; a.frame_stride = (long)frame_stride; a.frames = frames; a.lg = lg;
    a.f0 = f0; a.aper = aperiodicity; a.lag = lag; a.ws = (unsigned short*)workspace; a.ws_item = (long)(per_item / 2);
    a.T = T; a.tau_min = tau_min; a.tau_max = tau_max; a.sr = (float)sampling_rate;
    a.unvoiced_q = unvoiced_q; a.octave_q = octave_q; a.jump_q = jump_q; a.vuv_q = vuv_q;
    const int S = tau_max - tau_min;
    const int threads = min(VIT_MAX_THREADS, (S + 63) / 64 * 64);
    hipLaunchKernelGGL(viterbi_kernel, dim3((unsigned)B), dim3((unsigned)threads), 0, (hipStream_t)stream, a);
    return efts_check_launch(who);
}
