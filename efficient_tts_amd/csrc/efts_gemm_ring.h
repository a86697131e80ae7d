// efts_gemm_ring.h -- gemm_kernel, the ring kernel of efts_gemm (design: efts_gemm.hip), for every column tile width.
//
// A tile is a 128-row window x BNT columns; the four waves split it as
//     BNT = 128: 2 x 2 waves of 64 x 64      BNT = 64: 2 x 2 waves of 64 x 32      BNT = 32: 4 x 1 waves of 32 x 32
// so the 32- and 64-channel stages of the vocoder do not spend 4x / 2x of their MFMAs on clamped duplicate columns, and launches
// that would leave most CUs idle get twice the workgroups.  The weight tile shrinks with BNT (BNT / 32 DMA pieces per wave and
// step); window, ring, step loop and epilogue are the same code, and the K order per output element does not depend on BNT: the
// instantiations are bit-identical.  efts_gemm.hip instantiates BNT = 128, efts_gemm_narrow.hip BNT = 64 / 32.
#pragma once
#include "efts_gemm_epilogue.h"

namespace efts {

// Epilogue features per tile width: the extras (and the fp32 main loop, split 3) are compiled into the 128-column tiling alone.
template <int SPLIT, int BNT>
constexpr unsigned ring_features() { return BNT == 128 ? EPI_ALL | (SPLIT == 3 ? EPI_FP32 : 0u) : EPI_PLAIN; }

template <int TAPS, int SPLIT, int BNT, int DBG>
__global__ __launch_bounds__(256, 2) void gemm_kernel(GemmKernelArgs p) {
    static_assert(BNT == 128 || BNT == 64 || BNT == 32, "column tile");
    static_assert(BNT == 128 || (SPLIT != 3 && DBG == 0), "fp32 planes and the debug instantiations: 128-column tiles only");
    constexpr unsigned F = ring_features<SPLIT, BNT>();
    constexpr int WN = BNT == 32 ? 1 : 2;         // waves across the columns (4 / WN down the rows)
    constexpr int NI = BNT == 32 ? 1 : 2;         // 32-row accumulator blocks per wave
    constexpr int NJ = BNT == 128 ? 2 : 1;        // 32-column accumulator blocks per wave
    constexpr int WP = BNT / 32;                  // weight DMA pieces per wave and step
    constexpr int RPP = 1024 / BNT;               // tile rows per epilogue sweep: BNT / 4 threads per row
    constexpr int NPS = WIN / RPP;
    const int BM = p.bm;                      // output rows per tile: WIN - (TAPS - 1) * dilation
    unsigned long long pt[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long tq = 0;
#define EFTS_STAMP(i) do { if constexpr (DBG == 2) { const unsigned long long tn = __builtin_readcyclecounter(); pt[i] += tn - tq; tq = tn; } } while (0)
    extern __shared__ __attribute__((aligned(16))) char smem[];   // two window buffers, then the NST weight ring slots
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)((__attribute__((address_space(3))) char*)smem));

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int dbg = DBG ? p.dbg : 0;

    const int z = blockIdx.y;
    const int z2 = blockIdx.z;
    const int lrow = lane & 31;
    const int lhalf = lane >> 5;
    const int nsteps = p.nchunk * TAPS;
    const char* A = p.a + (long)z * p.a_bs + (long)z2 * p.a_bs2;
    const char* Bw = p.b + (long)z * p.b_bs + (long)z2 * p.b_bs2;

    // Workgroups walk the tile list with stride gridDim.x (one tile each by default).
    // XCD-aware tile order: block b runs on XCD b % 8; give each XCD a contiguous range of
    // tiles (n fastest) so the workgroups sharing an A window hit the same L2.
    const int ntot = p.mtiles * p.ntiles;
  for (int vt = blockIdx.x; vt < ntot; vt += gridDim.x) {
    int bid = vt;
    {
        const int q = ntot >> 3, r = ntot & 7;
        const int xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int mt = bid / p.ntiles, nt = bid - mt * p.ntiles;
    const int m0 = mt * BM, n0 = nt * BNT;
    const EpiTile et = epi_tile<BNT>(p, z, z2, m0, n0, WIN, BM);

    // per-lane DMA offsets of the 4 window pieces and WP weight pieces this wave issues per step:
    // piece pc covers tile rows 8*pc .. 8*pc+7; lane l -> row 8*pc + l/8, physical slot l%8
    unsigned voa[4], vow[WP];
    {
        const int b_max = p.n - 1 - n0;        // clamp B rows to the last real row
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (wave * 4 + q) * 8 + (lane >> 3);
            const int sl = (lane & 7) ^ ((r >> 1) & 7);
            voa[q] = (unsigned)(r * (int)p.lda + (sl << 4));
        }
#pragma unroll
        for (int q = 0; q < WP; ++q) {
            const int r = (wave * WP + q) * 8 + (lane >> 3);
            const int sl = (lane & 7) ^ ((r >> 1) & 7);
            vow[q] = (unsigned)((r < b_max ? r : b_max) * (int)p.ldb + (sl << 4));
        }
    }
    // debug bits 8 / 16 (timing experiments): every workgroup stages the SAME weight tile / window (always L1-resident)
    const bool alias_w = DBG && (dbg & 8), alias_a = DBG && (dbg & 16);
    const char* a_base = A + (long)((alias_a ? 0 : m0) - p.pad * p.dil) * p.lda;     // window row 0 (may start in the guard rows)
    const char* w_base = Bw + (long)(alias_w ? 0 : n0) * p.ldb;

    auto issue_w = [&](int cn, int kn, int slot) {     // weights of step (chunk cn, tap kn) -> ring slot
        if (alias_w) { cn = 0; kn = 0; }
        const char* sb = w_base + (long)kn * p.b_tap_stride + (long)cn * 128;
        const unsigned l = lds0 + 2 * TILE_BYTES + slot * TILE_BYTES + wave * WP * 1024;
#pragma unroll
        for (int q = 0; q < WP; ++q) dma16(l + q * 1024, vow[q], sb);
    };
    auto issue_a = [&](int cn) {     // A window of chunk cn -> window buffer cn & 1
        const char* sb = a_base + (long)(alias_a ? 0 : cn) * 128;
        const unsigned l = lds0 + wave * 4096 + (cn & 1) * TILE_BYTES;
#pragma unroll
        for (int q = 0; q < 4; ++q) dma16(l + q * 1024, voa[q], sb);
    };

    f32x16 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // MFMAs of one (chunk, tap) step: window buffer `ab`, weight ring slot `ws`, tap k
    auto compute = [&](int ab, int ws, int k) {
        const char* at = smem + ab * TILE_BYTES;
        const char* wt = smem + 2 * TILE_BYTES + ws * TILE_BYTES;
        const int arow = wm * (NI * 32) + lrow + k * p.dil;   // tile row of output row r at tap k is r + k * dilation
        const int brow = wn * (NJ * 32) + lrow;
        if (DBG && (dbg & 4)) return;
        // Operand fragments are double-buffered in registers: the ds_reads of k-slice kk+1 are issued
        // before the MFMAs of slice kk (scheduler fenced), so only the first slice's LDS latency is
        // exposed per step and the waits are counted lgkmcnt(N).
        if constexpr (SPLIT == 1) {
            bf16x8 af[2][NI], bfr[2][NJ];
            auto ld = [&](int kk, int b) {
                const int slot = kk * 2 + lhalf;
#pragma unroll
                for (int i = 0; i < NI; ++i) af[b][i] = *(const bf16x8*)(at + lds_off(arow + i * 32, slot));
#pragma unroll
                for (int j = 0; j < NJ; ++j) bfr[b][j] = *(const bf16x8*)(wt + lds_off(brow + j * 32, slot));
            };
            ld(0, 0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (kk + 1 < 4) ld(kk + 1, (kk + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[kk & 1][i], bfr[kk & 1][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else if constexpr (SPLIT == 3) {
            // fp32 planes (efts_abi.h split 3): a chunk row is 8 slots of 4 floats.  Lane half h reads slot 2q + h of each 32-row
            // fragment; MFMA (q, e) of v_mfma_f32_32x32x2_f32 takes element e of it, i.e. k = 8q + e (h = 0) and 8q + 4 + e (h = 1).
            // A and B are permuted alike, so the 16 MFMAs sum over all 32 k's; the four accumulators are independent (64-cycle latency).
            f32x4 af[2][NI], bfr[2][NJ];
            auto ld = [&](int q, int b) {
                const int slot = q * 2 + lhalf;
#pragma unroll
                for (int i = 0; i < NI; ++i) af[b][i] = *(const f32x4*)(at + lds_off(arow + i * 32, slot));
#pragma unroll
                for (int j = 0; j < NJ; ++j) bfr[b][j] = *(const f32x4*)(wt + lds_off(brow + j * 32, slot));
            };
            ld(0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q + 1 < 4) ld(q + 1, (q + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q & 1][i][e], bfr[q & 1][j][e], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            bf16x8 ah[2][NI], al[2][NI], bh[2][NJ], bl[2][NJ];
            auto ld = [&](int kk, int b) {
                const int slot = kk * 2 + lhalf;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    ah[b][i] = *(const bf16x8*)(at + lds_off(arow + i * 32, slot));
                    al[b][i] = *(const bf16x8*)(at + lds_off(arow + i * 32, slot + 4));
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    bh[b][j] = *(const bf16x8*)(wt + lds_off(brow + j * 32, slot));
                    bl[b][j] = *(const bf16x8*)(wt + lds_off(brow + j * 32, slot + 4));
                }
            };
            ld(0, 0);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                if (kk + 1 < 2) ld(kk + 1, (kk + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[kk & 1][i], bh[kk & 1][j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kk & 1][i], bl[kk & 1][j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[kk & 1][i], bh[kk & 1][j], acc[i][j], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // prologue: window 0, weights of steps 0 and 1; wait for window 0 + weights 0
    const bool dma_on = !(dbg & 2);
    if (dma_on) {
        issue_a(0);
        issue_w(0, 0, 0);
        if (nsteps > 1) issue_w(TAPS == 1 ? 1 : 0, TAPS == 1 ? 0 : 1, 1);
        wait_vmcnt<WP>(nsteps > 1 ? WP : 0);
    }
    __builtin_amdgcn_s_barrier();

    // (c, k): this step; (c2, k2): the step whose weights are issued now (two ahead); ws: ring slot of this step
    int c = 0, k = 0, ws = 0;
    int c2 = (TAPS == 1) ? 2 : (TAPS == 2 ? 1 : 0), k2 = (TAPS == 1) ? 0 : 2 % TAPS;
    for (int s = 0; s + 1 < nsteps; ++s) {
        if constexpr (DBG == 2) tq = __builtin_readcyclecounter();
        // ---- issue: weights two steps ahead; the next window at the first tap of a chunk.
        // taps 1: the window is needed one step later, so it goes out BEFORE the weights.
        const bool do_w = (s + 2 < nsteps) && dma_on;
        const bool do_a = (k == 0) && (c + 1 < p.nchunk) && dma_on;
        if (TAPS == 1 && do_a) issue_a(c + 1);
        if (do_w) issue_w(c2, k2, ws == 0 ? 2 : ws - 1);      // slot (s + 2) % 3
        if (TAPS != 1 && do_a) issue_a(c + 1);
        EFTS_STAMP(0);
        compute(c & 1, ws, k);
        EFTS_STAMP(2);
        // ---- step end: the operands of step s+1 must have landed.  LDS-DMA completes in issue
        // order, so it is enough to bound what may still be in flight: everything issued AFTER the
        // weights of s+1, i.e. this step's issues and (taps > 1) a window issued one step ago.
        int n = do_w ? WP : 0;
        if (TAPS != 1) {
            if (do_a) n += 4;
            if (k == 1 && c + 1 < p.nchunk && dma_on) n += 4;
        }
        wait_vmcnt<WP>(n);
        EFTS_STAMP(3);
        lds_barrier();
        EFTS_STAMP(4);
        if (++k == TAPS) { k = 0; ++c; }
        if (++k2 == TAPS) { k2 = 0; ++c2; }
        ws = (ws == 2) ? 0 : ws + 1;
    }

    // ---- last step: nothing left to stage.  The epilogue operands of this thread (NPS residual float4 + NPS row-mask
    // values) are requested first so that their HBM latency hides under the step's MFMAs and the LDS staging of the accumulators.
    u32x4 rres[NPS];
    float rmv[NPS];
    const bool pre = et.vec && !(dbg & 1);
    const auto rowof = [](int ps) { return ps * RPP; };
    if constexpr (DBG == 2) tq = __builtin_readcyclecounter();
    if (pre) epi_prefetch(p, et, rres, rmv, rowof);
    EFTS_STAMP(0);
    compute((p.nchunk - 1) & 1, ws, TAPS - 1);
    EFTS_STAMP(2);
    lds_barrier();
    EFTS_STAMP(4);

    // ---- fused epilogue (efts_gemm_epilogue.h): each wave drops its NI x NJ blocks into a [128][BNT] fp32 LDS tile, then BNT / 4
    // consecutive threads sweep one tile row
    float* cs = (float*)smem;   // at most 64 KiB; the main loop's last barrier has retired all LDS reads
    if constexpr (DBG == 2) tq = __builtin_readcyclecounter();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cl = wn * (NJ * 32) + j * 32 + lrow;
        const float bv = epi_bias(p, n0 + cl);
#pragma unroll
        for (int i = 0; i < NI; ++i) epi_stage<BNT, F>(p, cs, acc[i][j], wm * (NI * 32) + i * 32, cl, bv);
    }
    lds_barrier();
    if constexpr (F & EPI_SIDX) {
        if (p.sidx) {
            // softmax over the valid columns of every row + its expected column index, from the staged tile (32 threads per row, 4
            // columns each; the three reductions run over the 32 lanes of a half wave).  ntiles == 1: the tile holds whole rows.
            const int kl = min(p.klen[z], p.n), ql = min(p.qlen[z], p.m);
            const int c4 = et.c4;
            float* so = p.sidx + (long)z * p.m;
#pragma unroll 4
            for (int ps = 0; ps < NPS; ++ps) {
                const int rl = ps * RPP + (int)et.trow;
                const int row = m0 + rl;
                const float4 v = *(const float4*)(cs + rl * BNT + c4);
                const float vv[4] = {v.x, v.y, v.z, v.w};
                float mx = -INFINITY;
#pragma unroll
                for (int u = 0; u < 4; ++u) mx = (c4 + u < kl) ? fmaxf(mx, vv[u]) : mx;
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 32));
                float se = 0.f, si = 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float e = (c4 + u < kl) ? __expf(vv[u] - mx) : 0.f;
                    se += e;
                    si += e * (float)(c4 + u);
                }
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) { se += __shfl_xor(se, off, 32); si += __shfl_xor(si, off, 32); }
                if ((tid & 31) == 0 && rl < BM && row < p.m) so[row] = row < ql ? si / se : 0.f;
            }
        }
    }
    float part_sq = 0.f;
    if (pre) part_sq = epi_sweep_vec<BNT, RPP, NPS, NPS, F>(p, et, cs, rres, rmv, rowof);
    else if (et.col < p.n && !(dbg & 1)) epi_sweep_scalar<BNT, RPP, NPS, F>(p, et, cs, rowof);
    if constexpr (F & EPI_SQERR) {
        if (p.sqerr) {   // every wave adds its 64 shares up the same way (xor butterfly) and owns one slot: no atomics, no run-to-run difference
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) part_sq += __shfl_xor(part_sq, off, 64);
            if (lane == 0) p.sqerr[((long)z * ntot + bid) * 4 + wave] = part_sq;
        }
    }
    lds_barrier();   // the LDS tile is re-used by the next tile's operand ring; stores drain on their own
    if constexpr (DBG == 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        EFTS_STAMP(5);
    }
  }   // tile loop
    if constexpr (DBG == 2) {
        if (lane == 0 && p.prof) {
            for (int i = 0; i < 6; ++i) atomicAdd(p.prof + i, pt[i]);
            atomicAdd(p.prof + 6, 1ull);
        }
    }
#undef EFTS_STAMP
}

}  // namespace efts
