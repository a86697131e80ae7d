// efts_conv5.hip -- the k5 convolution of efts_gemm.hip on 256-row windows (two 4-wave workgroups per CU, 252 x 128 tiles):
// used for large bf16 k5 launches that keep an fp32 residual stream (the training step's forward and dgrad convolutions);
// the inference stacks run on efts_resconv5 (efts_resconv.hip).  Bit-identical to gemm_kernel on the same operands.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_gemm_epilogue.h"

namespace efts {

// =============================================================================================
// conv5_kernel: the k5 residual convolution at large M.  Same machinery as gemm_kernel, tiled like
// the direct wgrad kernel: a 256-row window (252 output rows) x 128 columns per workgroup, 2x2 waves
// of 128x64 (8 accumulator blocks = 128 VGPRs), FULL 128-byte rows.  Every 16 KiB weight tile now
// feeds 32 MFMAs per wave instead of 16, i.e. 0.58x the LDS-DMA line requests per FLOP.
// LDS: ONE 32 KiB window + the 3-stage weight ring = exactly 80 KiB (two workgroups per CU); the
// window of the next chunk can only be requested after the last tap has read the current one, so
// that latency is exposed once per chunk (every 5th step) and covered by the co-resident workgroup.
// The epilogue runs in two passes through the 64 KiB staging tile, each pass taking accumulator
// blocks i = 2*ep, 2*ep+1 of EVERY wave (all waves stage equally, half the accumulators die early).
// =============================================================================================

template <int SPLIT>
__global__ __launch_bounds__(256, 2) void conv5_kernel(GemmKernelArgs p) {
    constexpr int TAPS = 5;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)((__attribute__((address_space(3))) char*)smem));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int z = blockIdx.y;
    const int lrow = lane & 31, lhalf = lane >> 5;
    const int nsteps = p.nchunk * TAPS;
    constexpr int RPP = 8, NPS = 16, NRING = 8;
    const char* A = p.a + (long)z * p.a_bs;
    const char* Bw = p.b + (long)z * p.b_bs;
    const int ntot = p.mtiles * p.ntiles;
  for (int vt = blockIdx.x; vt < ntot; vt += gridDim.x) {
    int bid = vt;
    {
        const int q = ntot >> 3, r = ntot & 7;
        const int xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int mt = bid / p.ntiles, nt = bid - mt * p.ntiles;
    const int m0 = mt * C5_BM, n0 = nt * BN;
    const EpiTile et = epi_tile<BN>(p, z, 0, m0, n0, C5_WIN, C5_BM);

    unsigned voa[8], vow[4];      // per-lane DMA offsets: 8 window pieces + 4 weight pieces per wave
    {
        const int b_max = p.n - 1 - n0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = (wave * 8 + q) * 8 + (lane >> 3);
            const int sl = (lane & 7) ^ ((r >> 1) & 7);
            voa[q] = (unsigned)(r * (int)p.lda + (sl << 4));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (wave * 4 + q) * 8 + (lane >> 3);
            const int sl = (lane & 7) ^ ((r >> 1) & 7);
            vow[q] = (unsigned)((r < b_max ? r : b_max) * (int)p.ldb + (sl << 4));
        }
    }
    const char* a_base = A + (long)(m0 - 2) * p.lda;
    const char* w_base = Bw + (long)n0 * p.ldb;
    auto issue_w = [&](int cn, int kn, int slot) {
        const char* sb = w_base + (long)kn * p.b_tap_stride + (long)cn * 128;
        const unsigned l = lds0 + C5_A_BYTES + slot * TILE_BYTES + wave * 4096;
#pragma unroll
        for (int q = 0; q < 4; ++q) dma16(l + q * 1024, vow[q], sb);
    };
    auto issue_a = [&](int cn) {
        const char* sb = a_base + (long)cn * 128;
        const unsigned l = lds0 + wave * 8192;
#pragma unroll
        for (int q = 0; q < 8; ++q) dma16(l + q * 1024, voa[q], sb);
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int ws, int k) {
        const char* at = smem;
        const char* wt = smem + C5_A_BYTES + ws * TILE_BYTES;
        const int arow = wm * 128 + lrow + k;
        const int brow = wn * 64 + lrow;
        if constexpr (SPLIT == 1) {
            bf16x8 af[2][4], bfr[2][2];
            auto ld = [&](int kk, int b) {
                const int slot = kk * 2 + lhalf;
#pragma unroll
                for (int j = 0; j < 2; ++j) bfr[b][j] = *(const bf16x8*)(wt + lds_off(brow + j * 32, slot));
#pragma unroll
                for (int i = 0; i < 4; ++i) af[b][i] = *(const bf16x8*)(at + lds_off(arow + i * 32, slot));
            };
            ld(0, 0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (kk + 1 < 4) ld(kk + 1, (kk + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[kk & 1][i], bfr[kk & 1][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int slot = kk * 2 + lhalf;
                bf16x8 bh[2], bl[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    bh[j] = *(const bf16x8*)(wt + lds_off(brow + j * 32, slot));
                    bl[j] = *(const bf16x8*)(wt + lds_off(brow + j * 32, slot + 4));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bf16x8 ah = *(const bf16x8*)(at + lds_off(arow + i * 32, slot));
                    const bf16x8 al = *(const bf16x8*)(at + lds_off(arow + i * 32, slot + 4));
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[j], acc[i][j], 0, 0, 0);
                    }
                }
            }
        }
    };

    issue_a(0);
    issue_w(0, 0, 0);
    if (nsteps > 1) issue_w(0, 1, 1);
    wait_vmcnt(nsteps > 1 ? 4 : 0);
    __builtin_amdgcn_s_barrier();

    int c = 0, k = 0, ws = 0, c2 = 0, k2 = 2;
    for (int s = 0; s + 1 < nsteps; ++s) {
        const bool do_w = s + 2 < nsteps;
        if (do_w) issue_w(c2, k2, ws == 0 ? 2 : ws - 1);        // weights two steps ahead, slot (s + 2) % 3
        compute(ws, k);
        if (k == TAPS - 1) {
            lds_barrier();                                      // every wave has finished reading the window of chunk c
            issue_a(c + 1);
            wait_vmcnt(0);
        } else {
            wait_vmcnt(do_w ? 4 : 0);
        }
        lds_barrier();
        if (++k == TAPS) { k = 0; ++c; }
        if (++k2 == TAPS) { k2 = 0; ++c2; }
        ws = (ws == 2) ? 0 : ws + 1;
    }

    // ---- last step + epilogue (efts_gemm_epilogue.h), two passes through the 64 KiB staging tile: pass ep takes accumulator
    // blocks 2 * ep, 2 * ep + 1 of every wave, i.e. tile rows 64 * ep + (0 .. 63) and 128 + 64 * ep + (0 .. 63).  The operands of
    // the first 8 sweeps of a pass are requested ahead of its staging, the other 8 as the ring of 8 falls free.
    u32x4 rres[NRING];
    float rmv[NRING];
    compute(ws, TAPS - 1);
    lds_barrier();

    float* cs = (float*)smem;
#pragma unroll
    for (int ep = 0; ep < 2; ++ep) {
        const auto rowof = [ep](int ps) { return ps * RPP + 64 * ep + (ps >= 8 ? 64 : 0); };
        if (et.vec) epi_prefetch(p, et, rres, rmv, rowof);          // in flight while the accumulators are staged
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cl = wn * 64 + j * 32 + lrow;
            const float bv = epi_bias(p, n0 + cl);
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) epi_stage<BN, EPI_WIDE>(p, cs, acc[2 * ep + ii][j], wm * 64 + ii * 32, cl, bv);
        }
        lds_barrier();
        if (et.vec) epi_sweep_vec<BN, RPP, NPS, NRING, EPI_WIDE>(p, et, cs, rres, rmv, rowof);
        else if (et.col < p.n) epi_sweep_scalar<BN, RPP, NPS, EPI_WIDE>(p, et, cs, rowof);
        lds_barrier();
    }
  }   // tile loop
}


#ifdef EFTS_LAB
// =============================================================================================
// conv8_kernel (experiment, EFTS_CONV8=1): the k5 convolution with ONE 8-wave workgroup per CU on a 256-row x 256-column
// tile: 2 x 4 waves of 128 x 64 (conv5_kernel's wave tile), one 32 KiB window + a 3-stage ring of 32 KiB weight tiles =
// 128 KiB.  Half the weight DMA per MFMA of conv5_kernel, one barrier domain of 8 waves, two waves of the same
// workgroup per SIMD.  The epilogue goes through the 128 KiB in two column halves.  bf16 planes, n % 256 == 0.
// =============================================================================================

__global__ __launch_bounds__(512, 2) void conv8_kernel(GemmKernelArgs p) {
    constexpr int TAPS = 5;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)((__attribute__((address_space(3))) char*)smem));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int z = blockIdx.y;
    const int lrow = lane & 31, lhalf = lane >> 5;
    const int nsteps = p.nchunk * TAPS;
    const char* A = p.a + (long)z * p.a_bs;
    const char* Bw = p.b + (long)z * p.b_bs;
    const int ntot = p.mtiles * p.ntiles;
    int bid = blockIdx.x;
    {
        const int q = ntot >> 3, r = ntot & 7;
        const int xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int mt = bid / p.ntiles, nt = bid - mt * p.ntiles;
    const int m0 = mt * C5_BM, n0 = nt * C8_BN;

    unsigned voa[4], vow[4];      // per-lane DMA offsets: 4 window pieces + 4 weight pieces per wave
    {
        const int b_max = p.n - 1 - n0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (wave * 4 + q) * 8 + (lane >> 3);
            const int sl = (lane & 7) ^ ((r >> 1) & 7);
            voa[q] = (unsigned)(r * (int)p.lda + (sl << 4));
            vow[q] = (unsigned)((r < b_max ? r : b_max) * (int)p.ldb + (sl << 4));
        }
    }
    const char* a_base = A + (long)(m0 - 2) * p.lda;
    const char* w_base = Bw + (long)n0 * p.ldb;
    auto issue_w = [&](int cn, int kn, int slot) {
        const char* sb = w_base + (long)kn * p.b_tap_stride + (long)cn * 128;
        const unsigned l = lds0 + C5_A_BYTES + slot * C8_W_BYTES + wave * 4096;
#pragma unroll
        for (int q = 0; q < 4; ++q) dma16(l + q * 1024, vow[q], sb);
    };
    auto issue_a = [&](int cn) {
        const char* sb = a_base + (long)cn * 128;
        const unsigned l = lds0 + wave * 4096;
#pragma unroll
        for (int q = 0; q < 4; ++q) dma16(l + q * 1024, voa[q], sb);
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int ws, int k) {
        const char* at = smem;
        const char* wt = smem + C5_A_BYTES + ws * C8_W_BYTES;
        const int arow = wm * 128 + lrow + k;
        const int brow = wn * 64 + lrow;
        bf16x8 af[2][4], bfr[2][2];
        auto ld = [&](int kk, int b) {
            const int slot = kk * 2 + lhalf;
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[b][j] = *(const bf16x8*)(wt + lds_off(brow + j * 32, slot));
#pragma unroll
            for (int i = 0; i < 4; ++i) af[b][i] = *(const bf16x8*)(at + lds_off(arow + i * 32, slot));
        };
        ld(0, 0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kk + 1 < 4) ld(kk + 1, (kk + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[kk & 1][i], bfr[kk & 1][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    issue_a(0);
    issue_w(0, 0, 0);
    if (nsteps > 1) issue_w(0, 1, 1);
    wait_vmcnt(nsteps > 1 ? 4 : 0);
    __builtin_amdgcn_s_barrier();

    int c = 0, k = 0, ws = 0, c2 = 0, k2 = 2;
    for (int s = 0; s < nsteps; ++s) {
        const bool do_w = s + 2 < nsteps;
#ifndef C8_EXP
#define C8_EXP 0
#endif
        if (do_w && !(C8_EXP & 1)) issue_w(c2, k2, ws == 0 ? 2 : ws - 1);
        if (!(C8_EXP & 4)) compute(ws, k);
        if (k == TAPS - 1 && c + 1 < p.nchunk) {
            lds_barrier();                                      // every wave has finished reading the window of chunk c
            if (!(C8_EXP & 1)) issue_a(c + 1);
            if (!(C8_EXP & 2)) wait_vmcnt(0);
        } else {
            if (!(C8_EXP & 2)) wait_vmcnt(do_w ? 4 : 0);
        }
        if (!(C8_EXP & 8)) lds_barrier();
        if (++k == TAPS) { k = 0; ++c; }
        if (++k2 == TAPS) { k2 = 0; ++c2; }
        ws = (ws == 2) ? 0 : ws + 1;
    }

    // ---- epilogue (efts_gemm_epilogue.h): two column halves of 128 through [256][128] fp32 = 128 KiB; 32 threads per 512-byte
    // row, 16 rows a sweep, operands in a ring of 4.  The dispatcher sends aligned launches with n % 256 == 0 only: no scalar sweep.
    constexpr int RPP = 16, NPS = 16, NRING = 4;
    float* cs = (float*)smem;
    const auto rowof = [](int ps) { return ps * RPP; };
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        const EpiTile et = epi_tile<128>(p, z, 0, m0, n0 + h * 128, C5_WIN, C5_BM);
        u32x4 rres[NRING];
        float rmv[NRING];
        epi_prefetch(p, et, rres, rmv, rowof);
        if ((wn >> 1) == h) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int cl = (wn & 1) * 64 + j * 32 + lrow;
                const float bv = epi_bias(p, et.n0 + cl);
#pragma unroll
                for (int i = 0; i < 4; ++i) epi_stage<128, 0>(p, cs, acc[i][j], wm * 128 + i * 32, cl, bv);
            }
        }
        lds_barrier();
        epi_sweep_vec<128, RPP, NPS, NRING, 0>(p, et, cs, rres, rmv, rowof);
        lds_barrier();
    }
}

void launch_conv8(dim3 grid, hipStream_t st, const GemmKernelArgs& k) {
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)conv8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, C8_LDS); attr = true; }
    hipLaunchKernelGGL(conv8_kernel, grid, dim3(512), C8_LDS, st, k);
}
#endif

void launch_conv5_any(int split, dim3 grid, hipStream_t st, const GemmKernelArgs& k) {
    if (split == 1) hipLaunchKernelGGL((conv5_kernel<1>), grid, dim3(256), C5_LDS, st, k);
    else hipLaunchKernelGGL((conv5_kernel<2>), grid, dim3(256), C5_LDS, st, k);
}
void conv5_set_lds_attr() {
    (void)hipFuncSetAttribute((const void*)conv5_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, C5_LDS);
    (void)hipFuncSetAttribute((const void*)conv5_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, C5_LDS);
}

}  // namespace efts
