// efts_resblock2.hip -- one HiFi-GAN ResBlock2 (nntts/vocoders/hifigan_model.py:71-93) in one launch: two pre-activation turns
// x <- x + conv_{k,d}(leaky(x)) with the intermediate kept in LDS.  include/efts_abi.h has the definition; DESIGN.md the numbers.
//
// A workgroup (4 waves) owns bm = 32 nb - 2 h1 output rows (h0, h1: the halos (k - 1) / 2 * d of the two convolutions; nb <= 6 blocks of
// 32 rows, the most that fit the LDS, chosen on the host):
//   1. the window of the input plane P0, rows m0 - h1 - h0 .. m0 - h1 + 32 nb + h0, ALL K chunks, goes to LDS by plain 16-byte loads
//      (rows outside the row space are written as zeros and never read from memory);
//   2. first contraction: y1 on the 32 nb rows m0 - h1 .. (its rows plus the second halo), accumulators in registers; the epilogue
//      ((acc + bias) + x) * mask stays in the accumulator registers;
//   3. behind a barrier the window is dead: it is cleared and overwritten with P1 = plane(leaky(y1)) in the operand format of the
//      launch, and the bm central rows of y1 go to an fp32 tile behind it;
//   4. second contraction on P1, epilogue ((acc + bias) + y1) * mask in place in the fp32 tile, then a sweep of 16-byte stores.
// Blocks of 32 x 32 outputs: wave w owns column block w (c = 128), w % 2 (c = 64), or every column block (c <= 32, c = 96) and every
// (4 / waves across)-th row block.  The A fragments are ds_read_b128 from the swizzled window at the tap's row shift, the weight
// fragments come straight from global memory (a launch reads k * c rows of weights, L2-resident, each lane 64 contiguous bytes of a row
// per chunk and tap), requested one (chunk, tap) step ahead.  No barrier inside a contraction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_mma.h"

using namespace efts;

namespace {

constexpr int RB2_MAX_BLOCKS = 6;            // 32-row blocks of the first contraction per workgroup
constexpr int RB2_LDS_MAX = 160 * 1024;

struct Rb2Args {
    const float* x; const char* p0; const char* w0; const char* w1; const float* b0; const float* b1; const float* mask; float* out;
    long ldx, ldp, ldw, wts, ldo;
    int m, c, k, d0, d1, nchunk;
    int nb;          // 32-row blocks of the first contraction
    int bm;          // output rows per workgroup: 32 nb - 2 h1
    int w0rows;      // rows of the P0 window: 32 nb + 2 h0
    int ld;          // LDS bytes per window row: nchunk * 128
    int yoff;        // byte offset of the fp32 tile [bm][NC * 32]
    float slope;
};

template <int SPLIT, int NC>
__global__ __launch_bounds__(256) void resblock2_kernel(Rb2Args p) {
    constexpr int WN = NC == 4 ? 4 : (NC == 2 ? 2 : 1);      // waves across the column blocks
    constexpr int WM = 4 / WN;                               // ... down the row blocks
    constexpr int NJ = NC / WN;                              // column blocks per wave
    constexpr int MI = (RB2_MAX_BLOCKS + WM - 1) / WM;       // row blocks per wave, at the most
    constexpr int YW = NC * 32;                              // columns of the fp32 tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, lrow = lane & 31, lhalf = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int h0 = (p.k - 1) / 2 * p.d0, h1 = (p.k - 1) / 2 * p.d1;
    const int m0 = blockIdx.x * p.bm;
    const int g1 = m0 - h1;                                  // row of the row space at row 0 of the first contraction
    const int ld = p.ld;
    const bool key_full = (ld & 255) == 0;                   // rows r and r + 1 share banks: swizzle by r, else (128 mod 256) by r >> 1
    auto win_off = [&](int row, int chunk, int slot) { return row * ld + chunk * 128 + ((slot ^ ((key_full ? row : row >> 1) & 7)) << 4); };
    float* const yt = (float*)(smem + p.yoff);

    // ---- 1. the window of P0
    {
        const int spr = p.nchunk * 8, total = p.w0rows * spr;
        const int g0 = g1 - h0;
#pragma unroll 4
        for (int piece = tid; piece < total; piece += 256) {
            const int row = piece / spr, s = piece - row * spr;
            const int g = g0 + row;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (g >= 0 && g < p.m) v = *(const u32x4*)(p.p0 + (long)g * p.ldp + s * 16);
            *(u32x4*)(smem + win_off(row, s >> 3, s & 7)) = v;
        }
    }
    __syncthreads();

    int brow[NJ];                                            // the weight row of this lane per column block (clamped to the last real one)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = (wn + WN * j) * 32 + lrow;
        brow[j] = col < p.c ? col : p.c - 1;
    }
    f32x16 acc[MI][NJ];

    // one contraction: acc[i][j] = rows (wm + WM i) * 32 .. + 31 of the window at row shift tap * dil, columns of block wn + WN j
    auto contract = [&](const char* w, int dil, int nrb) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        u32x4 bc[NJ][4], bn[NJ][4];
        auto load_b = [&](u32x4 (&b)[NJ][4], int chunk, int tap) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const char* src = w + (long)tap * p.wts + (long)brow[j] * p.ldw + chunk * 128;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int slot = SPLIT == 2 ? 2 * (u & 1) + lhalf + 4 * (u >> 1) : 2 * u + lhalf;    // split 2: hi 0, hi 1, lo 0, lo 1
                    b[j][u] = *(const u32x4*)(src + slot * 16);
                }
            }
        };
        load_b(bc, 0, 0);
        const int nsteps = p.nchunk * p.k;
        int chunk = 0, tap = 0;
        for (int s = 0; s < nsteps; ++s) {
            int tn = tap + 1, cn = chunk;
            if (tn == p.k) { tn = 0; ++cn; }
            const bool more = s + 1 < nsteps;
            load_b(bn, more ? cn : chunk, more ? tn : tap);                 // in flight under this step's MFMAs
            const int shift = tap * dil;
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                if (wm + WM * i < nrb) {                                    // (wave-uniform)
                    const int arow = (wm + WM * i) * 32 + lrow + shift;
                    if constexpr (SPLIT == 1) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const bf16x8 fa = *(const bf16x8*)(smem + win_off(arow, chunk, 2 * u + lhalf));
#pragma unroll
                            for (int j = 0; j < NJ; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8, bc[j][u]), acc[i][j], 0, 0, 0);
                        }
                    } else if constexpr (SPLIT == 2) {
#pragma unroll
                        for (int kk = 0; kk < 2; ++kk) {
                            const bf16x8 ah = *(const bf16x8*)(smem + win_off(arow, chunk, 2 * kk + lhalf));
                            const bf16x8 al = *(const bf16x8*)(smem + win_off(arow, chunk, 2 * kk + lhalf + 4));
#pragma unroll
                            for (int j = 0; j < NJ; ++j) {                  // the order of efts_gemm inside a k-slice: lo*hi, hi*lo, hi*hi
                                const bf16x8 bh = __builtin_bit_cast(bf16x8, bc[j][kk]), bl = __builtin_bit_cast(bf16x8, bc[j][2 + kk]);
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[i][j], 0, 0, 0);
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[i][j], 0, 0, 0);
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[i][j], 0, 0, 0);
                            }
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {                       // lane half h holds k = 8 q + 4 h + e of the chunk in element e
                            const f32x4 fa = *(const f32x4*)(smem + win_off(arow, chunk, 2 * q + lhalf));
#pragma unroll
                            for (int e = 0; e < 4; ++e)
#pragma unroll
                                for (int j = 0; j < NJ; ++j)
                                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], __builtin_bit_cast(f32x4, bc[j][q])[e], acc[i][j], 0, 0, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int u = 0; u < 4; ++u) bc[j][u] = bn[j][u];
            chunk = cn; tap = tn;
        }
    };

    // ---- 2. y1 on rows g1 .. g1 + 32 nb - 1, left in the accumulator registers
    contract(p.w0, p.d0, p.nb);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        if (wm + WM * i < p.nb) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = (wn + WN * j) * 32 + lrow;
                const bool colok = col < p.c;
                const float bv = (colok && p.b0) ? p.b0[col] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int g = g1 + (wm + WM * i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                    const bool ok = colok && g >= 0 && g < p.m;
                    float v = 0.f;
                    if (ok) {
                        const float rm = p.mask ? p.mask[g] : 1.f;
                        v = ((acc[i][j][r] + bv) + p.x[(long)g * p.ldx + col]) * rm;
                    }
                    acc[i][j][r] = v;
                }
            }
        }
    }
    __syncthreads();                                         // every wave has read the last of P0

    // ---- 3. P1 over the window (cleared first: the padding k's of a chunk and the rows behind block nb - 1 read as zeros)
    {
        const int total = (p.nb + 1) * 32 * ld / 16;
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int piece = tid; piece < total; piece += 256) *(u32x4*)(smem + piece * 16) = z;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        if (wm + WM * i < p.nb) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = (wn + WN * j) * 32 + lrow;
                const int off = (int)plane_off_hi(col, SPLIT);
                const int chunk = off >> 7, slot = (off & 127) >> 4, sub = off & 15;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (wm + WM * i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                    const float y1 = acc[i][j][r];
                    const float v = y1 > 0.f ? y1 : y1 * p.slope;
                    if constexpr (SPLIT == 3) {
                        *(float*)(smem + win_off(row, chunk, slot) + sub) = v;
                    } else {
                        const unsigned short hi = f32_to_bf16(v);
                        *(unsigned short*)(smem + win_off(row, chunk, slot) + sub) = hi;
                        if constexpr (SPLIT == 2) *(unsigned short*)(smem + win_off(row, chunk, slot + 4) + sub) = f32_to_bf16(v - bf16_to_f32(hi));
                    }
                    const int r2 = row - h1;
                    if (r2 >= 0 && r2 < p.bm) yt[r2 * YW + col] = y1;
                }
            }
        }
    }
    __syncthreads();

    // ---- 4. y2 on rows m0 .. m0 + bm - 1
    const int nrb2 = (p.bm + 31) >> 5;
    contract(p.w1, p.d1, nrb2);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        if (wm + WM * i < nrb2) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = (wn + WN * j) * 32 + lrow;
                const float bv = (col < p.c && p.b1) ? p.b1[col] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int r2 = (wm + WM * i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                    const int g = m0 + r2;
                    if (r2 < p.bm && g < p.m) {
                        const float rm = p.mask ? p.mask[g] : 1.f;
                        yt[r2 * YW + col] = ((acc[i][j][r] + bv) + yt[r2 * YW + col]) * rm;       // (y1 came from another lane, behind the barrier above; in this step the element has one owner)
                    }
                }
            }
        }
    }
    __syncthreads();
    {
        const int rows_out = p.m - m0 < p.bm ? p.m - m0 : p.bm;
        const int c4 = p.c >> 2, total = rows_out * c4;
        const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out + (long)m0 * p.ldo, (long)rows_out * p.ldo * 4);
        for (int piece = tid; piece < total; piece += 256) {
            const int row = piece / c4, q = piece - row * c4;
            const u32x4 v = *(const u32x4*)(yt + row * YW + q * 4);
            store_b128(v, ro, (unsigned)(row * (int)p.ldo * 4 + q * 16), 0);      // (efts_mma.h: the data registers stay live behind the store)
        }
    }
}

template <int S, int NC>
void rb2_launch(int tiles, int lds, hipStream_t st, const Rb2Args& k) {
    static bool attr = false;
    if (!attr) { (void)hipFuncSetAttribute((const void*)resblock2_kernel<S, NC>, hipFuncAttributeMaxDynamicSharedMemorySize, RB2_LDS_MAX); attr = true; }
    hipLaunchKernelGGL((resblock2_kernel<S, NC>), dim3(tiles), dim3(256), lds, st, k);
}
template <int S>
void rb2_launch_nc(int nc, int tiles, int lds, hipStream_t st, const Rb2Args& k) {
    switch (nc) {
        case 1: rb2_launch<S, 1>(tiles, lds, st, k); break;
        case 2: rb2_launch<S, 2>(tiles, lds, st, k); break;
        case 3: rb2_launch<S, 3>(tiles, lds, st, k); break;
        default: rb2_launch<S, 4>(tiles, lds, st, k);
    }
}

}  // namespace

extern "C" int efts_resblock2(const efts_resblock2_args* a, void* stream) {
    if (!a) return efts_fail(EFTS_EINVAL, "efts_resblock2: null args");
    if (!(a->split >= EFTS_SPLIT_BF16 && a->split <= EFTS_SPLIT_FP32)) return efts_fail(EFTS_EINVAL, "efts_resblock2: split must be 1, 2 or 3");
    if (!(a->k == 3 || a->k == 5 || a->k == 7 || a->k == 9 || a->k == 11)) return efts_fail(EFTS_EINVAL, "efts_resblock2: k must be 3, 5, 7, 9 or 11");
    if (a->m <= 0) return efts_fail(EFTS_ESHAPE, "efts_resblock2: m must be positive");
    if (a->c < 4 || a->c > 128 || a->c % 4) return efts_fail(EFTS_ESHAPE, "efts_resblock2: c must be a multiple of 4 in 4 .. 128");
    if (a->reserved != 0) return efts_fail(EFTS_EINVAL, "efts_resblock2: reserved must be 0");
    if (a->d0 < 1 || a->d1 < 1 || a->d0 > 64 || a->d1 > 64) return efts_fail(EFTS_ESHAPE, "efts_resblock2: dilations must lie in 1 .. 64");
    const int h0 = (a->k - 1) / 2 * a->d0, h1 = (a->k - 1) / 2 * a->d1;
    if (h0 + h1 > 64) return efts_fail(EFTS_ESHAPE, "efts_resblock2: (k - 1) / 2 * (d0 + d1) must not exceed 64 rows");
    if (!a->x || !a->p0 || !a->w0 || !a->w1 || !a->out) return efts_fail(EFTS_EINVAL, "efts_resblock2: null operand");
    const int nchunk = (a->c + (a->split == 1 ? 63 : 31)) / (a->split == 1 ? 64 : 32);
    if (a->ldx < a->c || a->ldo < a->c || a->ldp < (int64_t)nchunk * 128 || a->ldw < (int64_t)nchunk * 128 || a->w_tap_stride < (int64_t)a->c * a->ldw)
        return efts_fail(EFTS_ESHAPE, "efts_resblock2: a row stride smaller than the row (or a tap stride smaller than c weight rows)");
    if (a->ldx > (1 << 20) || a->ldo > (1 << 20) || a->ldp > (1 << 23) || a->ldw > (1 << 23)) return efts_fail(EFTS_ESHAPE, "efts_resblock2: row stride too large");
    if (((uintptr_t)a->x & 15) || ((uintptr_t)a->p0 & 15) || ((uintptr_t)a->w0 & 15) || ((uintptr_t)a->w1 & 15) || ((uintptr_t)a->out & 15) ||
        (a->ldx & 3) || (a->ldo & 3) || (a->ldp & 15) || (a->ldw & 15) || (a->w_tap_stride & 15))
        return efts_fail(EFTS_EALIGN, "efts_resblock2: x, p0, w0, w1, out and their row / tap strides must be 16-byte aligned");

    Rb2Args k;
    k.x = a->x; k.p0 = (const char*)a->p0; k.w0 = (const char*)a->w0; k.w1 = (const char*)a->w1; k.b0 = a->bias0; k.b1 = a->bias1; k.mask = a->rowmask; k.out = a->out;
    k.ldx = a->ldx; k.ldp = a->ldp; k.ldw = a->ldw; k.wts = a->w_tap_stride; k.ldo = a->ldo;
    k.m = a->m; k.c = a->c; k.k = a->k; k.d0 = a->d0; k.d1 = a->d1; k.nchunk = nchunk; k.slope = a->slope;
    k.ld = nchunk * 128;
    const int nc = (a->c + 31) / 32;
    // the most 32-row blocks whose window, intermediate and fp32 tile fit the LDS (h0 + h1 <= 64: two blocks always fit where they are needed)
    int lds = 0;
    k.nb = 0;
    for (int nb = RB2_MAX_BLOCKS; nb >= 1; --nb) {
        const int bm = 32 * nb - 2 * h1;
        if (bm < 8) break;
        const int w0rows = 32 * nb + 2 * h0, rows = w0rows > 32 * (nb + 1) ? w0rows : 32 * (nb + 1);
        const int need = rows * k.ld + bm * nc * 32 * 4;
        if (need <= RB2_LDS_MAX) { k.nb = nb; k.bm = bm; k.w0rows = w0rows; k.yoff = rows * k.ld; lds = need; break; }
    }
    if (!k.nb) return efts_fail(EFTS_ESHAPE, "efts_resblock2: no tile fits the LDS for k %d, dilations %d and %d, c %d", a->k, a->d0, a->d1, a->c);
    const int tiles = (a->m + k.bm - 1) / k.bm;
    hipStream_t st = (hipStream_t)stream;
    if (a->split == 1) rb2_launch_nc<1>(nc, tiles, lds, st, k);
    else if (a->split == 2) rb2_launch_nc<2>(nc, tiles, lds, st, k);
    else rb2_launch_nc<3>(nc, tiles, lds, st, k);
    return efts_check_launch("efts_resblock2");
}
