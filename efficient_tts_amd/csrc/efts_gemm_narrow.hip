// efts_gemm_narrow.hip -- the MFMA contraction of efts_gemm.hip on narrow column tiles (see that file for the design):
// the 64- / 32-column instantiations of gemm_kernel (efts_gemm_ring.h: outputs of at most 64 columns, and launches that would
// leave most CUs idle) and resident32_kernel (one K chunk, <= 64 columns, many rows: window and all taps resident in LDS).
// Both are bit-identical to the 128-column gemm_kernel on the same operands.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_gemm_ring.h"

namespace efts {

// =============================================================================================
// resident32_kernel: convolutions with ONE K chunk (cin <= 64 bf16 / 32 bf16x3) and at most 32 output columns -- the
// 32-channel stage of the vocoder, 1.6 M rows at a batch of 8.  There the ring kernels are all overhead: 124 rows per
// workgroup, a window wait, one barrier per tap, an epilogue, for 44 MFMAs per wave.  Here a workgroup keeps a 256-row
// window AND the weights of every tap in LDS (32 KiB + taps x 4 KiB <= 76 KiB: two workgroups per CU): everything is
// requested up front, one wait, one barrier, then all taps back to back (wave = 64 rows x 32 columns) and the usual
// staged epilogue.  Same K order per output element as gemm_kernel (bit-compatible).
// =============================================================================================

template <int TAPS, int SPLIT>
__global__ __launch_bounds__(256, 2) void resident32_kernel(GemmKernelArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)((__attribute__((address_space(3))) char*)smem));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int z = blockIdx.y;
    const int lrow = lane & 31, lhalf = lane >> 5;
    const int BM = p.bm;                                       // R32_WIN - (TAPS - 1) * dilation
    const char* A = p.a + (long)z * p.a_bs;
    const char* Bw = p.b + (long)z * p.b_bs;
    const int mt = blockIdx.x / p.ntiles, nt = blockIdx.x - mt * p.ntiles;    // column tiles of 32 (n fastest: they share the window in L2)
    const int m0 = mt * BM, n0 = nt * 32;
    const int w0 = m0 - p.pad * p.dil;                         // first row of the window (may lie in the guard rows)
    const int row_max = p.m + 143;                             // last row the ABI lets us read (144 zero guard rows)

    // ---- request everything: 8 window pieces per wave, then this wave's piece (8 weight rows) of every tap
    {
        const char* a_base = A + (long)w0 * p.lda;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = (wave * 8 + q) * 8 + (lane >> 3);
            const int sl = (lane & 7) ^ ((r >> 1) & 7);
            const int rc = w0 + r > row_max ? row_max - w0 : r;   // rows past the guard read the last (zero) guard row
            dma16(lds0 + (wave * 8 + q) * 1024, (unsigned)(rc * (int)p.lda + (sl << 4)), a_base);
        }
        const int r = wave * 8 + (lane >> 3);
        const int sl = (lane & 7) ^ ((r >> 1) & 7);
        const int b_max = p.n - 1 - n0;
        const unsigned vw = (unsigned)((r < b_max ? r : b_max) * (int)p.ldb + (sl << 4));
        const char* w_base = Bw + (long)n0 * p.ldb;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) dma16(lds0 + R32_WIN * 128 + (k * 4 + wave) * 1024, vw, w_base + (long)k * p.b_tap_stride);
    }
    // epilogue operands of this thread (8 sweeps of 32 rows, 8 threads per 128-byte row): in flight under the DMA wait
    constexpr int RPP = 32, NPS = R32_WIN / RPP;
    const EpiTile et = epi_tile<32>(p, z, 0, m0, n0, R32_WIN, BM);
    const auto rowof = [](int ps) { return ps * RPP; };
    u32x4 rres[NPS];
    float rmv[NPS];
    if (et.vec) epi_prefetch(p, et, rres, rmv, rowof);

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    {
        const char* at = smem;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const char* wt = smem + R32_WIN * 128 + k * 4096;
            const int arow = wave * 64 + lrow + k * p.dil;
            if constexpr (SPLIT == 1) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int slot = kk * 2 + lhalf;
                    const bf16x8 b = *(const bf16x8*)(wt + lds_off(lrow, slot));
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const bf16x8 a = *(const bf16x8*)(at + lds_off(arow + i * 32, slot));
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[i], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const int slot = kk * 2 + lhalf;
                    const bf16x8 bh = *(const bf16x8*)(wt + lds_off(lrow, slot));
                    const bf16x8 bl = *(const bf16x8*)(wt + lds_off(lrow, slot + 4));
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const bf16x8 ah = *(const bf16x8*)(at + lds_off(arow + i * 32, slot));
                        const bf16x8 al = *(const bf16x8*)(at + lds_off(arow + i * 32, slot + 4));
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[i], 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[i], 0, 0, 0);
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[i], 0, 0, 0);
                    }
                }
            }
        }
    }
    lds_barrier();                                             // every wave is done with the window: it becomes the staging tile

    float* cs = (float*)smem;                                  // [256][32] fp32 = 32 KiB
    const float bv = epi_bias(p, n0 + lrow);
#pragma unroll
    for (int i = 0; i < 2; ++i) epi_stage<32, EPI_PLAIN>(p, cs, acc[i], wave * 64 + i * 32, lrow, bv);
    lds_barrier();
    if (et.vec) epi_sweep_vec<32, RPP, NPS, NPS, EPI_PLAIN>(p, et, cs, rres, rmv, rowof);
    else if (et.col < p.n) epi_sweep_scalar<32, RPP, NPS, EPI_PLAIN>(p, et, cs, rowof);
}


template <int T, int S, int B>
static void launch_narrow(dim3 grid, hipStream_t st, const GemmKernelArgs& k) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)gemm_kernel<T, S, B, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS);
        attr = true;
    }
    hipLaunchKernelGGL((gemm_kernel<T, S, B, 0>), grid, dim3(256), GEMM_LDS, st, k);
}
template <int T, int S>
static void launch_resident32(dim3 grid, hipStream_t st, const GemmKernelArgs& k) {
    static bool attr = false;
    constexpr int lds = R32_WIN * 128 + T * 4096;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)resident32_kernel<T, S>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr = true;
    }
    hipLaunchKernelGGL((resident32_kernel<T, S>), grid, dim3(256), lds, st, k);
}
template <int S>
static bool launch_resident32_taps(int taps, dim3 grid, hipStream_t st, const GemmKernelArgs& k) {
    switch (taps) {
        case 3: launch_resident32<3, S>(grid, st, k); return true;
        case 7: launch_resident32<7, S>(grid, st, k); return true;
        case 11: launch_resident32<11, S>(grid, st, k); return true;
        default: return false;
    }
}
template <int S, int B>
static bool launch_narrow_taps(int taps, dim3 grid, hipStream_t st, const GemmKernelArgs& k) {
    switch (taps) {
        case 1: launch_narrow<1, S, B>(grid, st, k); return true;
        case 3: launch_narrow<3, S, B>(grid, st, k); return true;
        case 5: launch_narrow<5, S, B>(grid, st, k); return true;
        case 7: launch_narrow<7, S, B>(grid, st, k); return true;
        case 11: launch_narrow<11, S, B>(grid, st, k); return true;
        default: return false;
    }
}

bool launch_narrow_any(int split, int bnt, int taps, dim3 grid, hipStream_t st, const GemmKernelArgs& k) {
    if (bnt == 32) return split == 1 ? launch_narrow_taps<1, 32>(taps, grid, st, k) : launch_narrow_taps<2, 32>(taps, grid, st, k);
    return split == 1 ? launch_narrow_taps<1, 64>(taps, grid, st, k) : launch_narrow_taps<2, 64>(taps, grid, st, k);
}
bool launch_resident32_any(int split, int taps, dim3 grid, hipStream_t st, const GemmKernelArgs& k) {
    return split == 1 ? launch_resident32_taps<1>(taps, grid, st, k) : launch_resident32_taps<2>(taps, grid, st, k);
}

}  // namespace efts
