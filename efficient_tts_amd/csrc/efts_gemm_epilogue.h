// efts_gemm_epilogue.h -- the fused row-sweep epilogue of the efts_gemm kernels, written once.
//
// Every tiling ends the same way.  Each wave drops its 32x32 accumulator blocks (alpha, bias, activation applied) into an fp32
// LDS tile of COLS columns (C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)), so
// that every global access is a full-row vector: after a barrier COLS / 4 consecutive threads sweep one tile row, RPP rows per
// sweep, NPS sweeps.  The residual and row-mask values of a sweep sit in registers, requested ahead of the last MFMAs.
// Addressing: raw buffer descriptors per tile, one per-thread byte offset, the sweep's tile row in the scalar offset; rows past
// the end of the matrix (or past the rows the tile owns, for the stores) fall outside the descriptor, so loads return 0 and
// stores are dropped without a per-row predicate.  Stores are never waited for.
//
// The order of floating-point operations per output element is the same in every tiling -- that is what makes them
// bit-identical -- and is written down here only:
//     acc * alpha + bias -> activation -> dropout scale -> (v + resid) * rowmask -> [fp32 store]
//                        -> plane_act -> hi = bf16(v), lo = bf16(v - hi) -> [plane stores]
#pragma once
#include "efts_gemm_kernels.h"

namespace efts {

// What an instantiation's epilogue can do.  The dispatcher of efts_gemm keeps a launch that needs a feature away from the
// tilings compiled without it (`generic_only` / `no_narrow` there).
enum : unsigned {
    EPI_TANH = 1,        // EFTS_ACT_TANH
    EPI_PLANE_ACT = 2,   // LeakyReLU on the way into the operand plane
    EPI_SIGN = 4,        // sign words of the activated value (128-column tiles: one 32-bit word per thread row and column phase)
    EPI_DROP = 8,        // train-mode dropout
    EPI_LO = 16,         // out_lo: the bf16 remainder in a plane of its own
    EPI_SQERR = 32,      // squared error against a target that travels where the residual would
    EPI_SIDX = 64,       // soft index of the row softmax (in the ring kernel, between staging and sweep)
    EPI_FP32 = 128,      // the operand plane holds unrounded fp32 (split 3)
};
constexpr unsigned EPI_PLAIN = EPI_TANH | EPI_PLANE_ACT;                           // 64- / 32-column ring tiles, resident32_kernel
constexpr unsigned EPI_WIDE = EPI_SIGN | EPI_DROP;                                 // conv5_kernel
constexpr unsigned EPI_ALL = EPI_PLAIN | EPI_WIDE | EPI_LO | EPI_SQERR | EPI_SIDX; // 128-column ring tiles

// One thread's view of one output tile of COLS columns: COLS / 4 threads per tile row, 4 columns each.
struct EpiTile {
    const float* resid;      // this batch item's residual (or loss target), row mask and outputs; null = absent
    const float* rowmask;
    float* of;
    char* ob;
    char* obl;
    int m0, n0;              // first row / column of the tile
    int rows_in, rows_out;   // rows of the matrix inside the tile's window / among the bm rows the tile owns
    int bm;
    int c4, col;             // the thread's first column inside the tile / of the matrix
    unsigned trow;           // its row inside a sweep
    bool vec;                // the vector sweep serves it: 16-byte aligned rows, four real columns
};
template <int COLS>
__device__ __forceinline__ EpiTile epi_tile(const GemmKernelArgs& p, int z, int z2, int m0, int n0, int win, int bm) {
    constexpr int TPR = COLS / 4;
    const int tid = threadIdx.x;
    EpiTile t;
    t.resid = p.resid ? p.resid + (long)z * p.r_bs : nullptr;
    t.rowmask = p.rowmask ? p.rowmask + (long)z * p.m_bs : nullptr;
    t.of = p.out_f32 ? p.out_f32 + (long)z * p.o_bs + (long)z2 * p.o_bs2 : nullptr;
    t.ob = p.out_bf16 ? p.out_bf16 + (long)z * p.ob_bs : nullptr;
    t.obl = p.out_lo ? p.out_lo + (long)z * p.ob_bs : nullptr;
    t.m0 = m0; t.n0 = n0; t.bm = bm;
    t.rows_in = p.m - m0 < win ? p.m - m0 : win;
    t.rows_out = p.m - m0 < bm ? p.m - m0 : bm;
    t.c4 = (tid % TPR) << 2;
    t.col = n0 + t.c4;
    t.trow = tid / TPR;
    t.vec = p.vec_ok && (t.col + 3 < p.n);
    return t;
}

__device__ __forceinline__ float epi_bias(const GemmKernelArgs& p, int c) { return (p.bias && c < p.n) ? p.bias[c] : 0.f; }

template <unsigned F>
__device__ __forceinline__ float epi_activate(const GemmKernelArgs& p, float acc, float bv) {
    float v = acc * p.alpha + bv;
    if (p.act == EFTS_ACT_LEAKY) v = v > 0.f ? v : v * p.slope;
    else if (p.act == EFTS_ACT_RELU) v = v > 0.f ? v : 0.f;
    else if ((F & EPI_TANH) && p.act == EFTS_ACT_TANH) v = tanhf(v);
    return v;
}
__device__ __forceinline__ float epi_resid_mask(float v, float x, float rm) { return (v + x) * rm; }

// Stage one 32x32 accumulator block at tile rows rl0 .. rl0 + 31, tile column cl (the lane's), with the column's bias bv.
template <int COLS, unsigned F>
__device__ __forceinline__ void epi_stage(const GemmKernelArgs& p, float* cs, const f32x16& acc, int rl0, int cl, float bv) {
    const int lhalf = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) cs[(rl0 + (r & 3) + 8 * (r >> 2) + 4 * lhalf) * COLS + cl] = epi_activate<F>(p, acc[r], bv);
}

// Sweep ps covers tile rows rowof(ps) + (0 .. RPP - 1) and holds its operands in slot ps % NRING.
template <int NRING>
__device__ __forceinline__ void epi_request(const GemmKernelArgs& p, const EpiTile& t, u32x4 (&res)[NRING], float (&rm)[NRING], int ps, int row0) {
    const __amdgpu_buffer_rsrc_t rr = make_rsrc(t.resid ? t.resid + (long)t.m0 * p.ldr : nullptr, t.resid ? (long)t.rows_in * p.ldr * 4 : 0);
    const __amdgpu_buffer_rsrc_t rk = make_rsrc(t.rowmask ? t.rowmask + t.m0 : nullptr, t.rowmask ? (long)t.rows_in * 4 : 0);
    res[ps % NRING] = __builtin_amdgcn_raw_buffer_load_b128(rr, t.trow * (unsigned)p.ldr * 4 + t.col * 4, row0 * (unsigned)p.ldr * 4, EFTS_AUX_LD);
    rm[ps % NRING] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rk, t.trow * 4, row0 * 4, 0));
}
// The residual / row-mask operands of the first NRING sweeps (t.vec threads only).
template <int NRING, class RowOf>
__device__ __forceinline__ void epi_prefetch(const GemmKernelArgs& p, const EpiTile& t, u32x4 (&res)[NRING], float (&rm)[NRING], RowOf rowof) {
#pragma unroll
    for (int ps = 0; ps < NRING; ++ps) epi_request(p, t, res, rm, ps, rowof(ps));
}

// The vector sweep (t.vec threads only; sign words: every lane of the wave).  NRING < NPS: the operands of sweep ps + NRING are
// requested as slot ps % NRING falls free.  Returns the thread's share of the squared error (EPI_SQERR, sweeps in ascending order).
template <int COLS, int RPP, int NPS, int NRING, unsigned F, class RowOf>
__device__ __forceinline__ float epi_sweep_vec(const GemmKernelArgs& p, const EpiTile& t, const float* cs, u32x4 (&res)[NRING], float (&rmv)[NRING],
                                               RowOf rowof) {
    static_assert(!(F & EPI_SIGN) || COLS == 128, "a sign word is the ballot of the 32 threads of one tile row");
    const int tid = threadIdx.x;
    const int osp = (F & EPI_FP32) ? EFTS_SPLIT_FP32 : (p.out_split == 2 ? 2 : 1);    // plane format of out_bf16
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(t.of ? t.of + (long)t.m0 * p.ldo : nullptr, t.of ? (long)t.rows_out * p.ldo * 4 : 0);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(t.ob ? t.ob + (long)t.m0 * p.ldob : nullptr, t.ob ? (long)t.rows_out * p.ldob : 0);
    const __amdgpu_buffer_rsrc_t rbl = make_rsrc(t.obl ? t.obl + (long)t.m0 * p.ldob : nullptr, t.obl ? (long)t.rows_out * p.ldob : 0);
    const unsigned ld_sg = (unsigned)(p.n >> 3);
    const __amdgpu_buffer_rsrc_t rsg = make_rsrc(p.sign ? p.sign + (long)t.m0 * ld_sg : nullptr, p.sign ? (long)t.rows_out * ld_sg : 0);
    const unsigned vo = t.trow * (unsigned)p.ldo * 4 + t.col * 4;
    const unsigned vb = t.trow * (unsigned)p.ldob + (unsigned)plane_off_hi(t.col, osp);
    const bool has_mask = t.rowmask != nullptr;
    float sq = 0.f;
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
        const unsigned row0 = rowof(ps);
        float4 v = *(const float4*)(cs + (ps * RPP + t.trow) * COLS + t.c4);
        if constexpr (F & EPI_SIGN) {
            if (p.sign) {                                    // (n % 128 == 0: every lane of the wave is here)
                const unsigned long long b0 = __ballot(v.x > 0.f), b1 = __ballot(v.y > 0.f), b2 = __ballot(v.z > 0.f), b3 = __ballot(v.w > 0.f);
                if ((tid & 31) == 0) {                       // lanes 0 / 32: the two rows this wave sweeps
                    const int sh = tid & 32;
                    const u32x4 w = {(unsigned)(b0 >> sh), (unsigned)(b1 >> sh), (unsigned)(b2 >> sh), (unsigned)(b3 >> sh)};
                    store_b128(w, rsg, t.trow * ld_sg + (unsigned)(t.n0 >> 7) * 16, row0 * ld_sg);
                }
            }
        }
        if constexpr (F & EPI_DROP) {
            if (p.drop_thresh) {                             // on the activated value, in front of the residual add
                const unsigned e0 = (unsigned)(t.m0 + row0 + t.trow) * (unsigned)p.n + t.col;
                v.x *= drop_scale(p.drop_seed_h, e0, p.drop_thresh, p.drop_inv_keep); v.y *= drop_scale(p.drop_seed_h, e0 + 1, p.drop_thresh, p.drop_inv_keep);
                v.z *= drop_scale(p.drop_seed_h, e0 + 2, p.drop_thresh, p.drop_inv_keep); v.w *= drop_scale(p.drop_seed_h, e0 + 3, p.drop_thresh, p.drop_inv_keep);
            }
        }
        const u32x4 x = res[ps % NRING];
        const float rm = has_mask ? rmv[ps % NRING] : 1.f;
        if constexpr (NRING < NPS) {
            if (ps + NRING < NPS) epi_request(p, t, res, rmv, ps + NRING, rowof(ps + NRING));
        }
        bool target = false;
        if constexpr (F & EPI_SQERR) target = p.sqerr != nullptr;
        if (target) {                                        // `resid` carries the loss target, not a residual (rows past the matrix: rm = 0)
            v.x *= rm; v.y *= rm; v.z *= rm; v.w *= rm;
            if (rm != 0.f) {
                const float d0 = v.x - __uint_as_float(x.x), d1 = v.y - __uint_as_float(x.y), d2 = v.z - __uint_as_float(x.z), d3 = v.w - __uint_as_float(x.w);
                sq += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
            }
        } else {
            v.x = epi_resid_mask(v.x, __uint_as_float(x.x), rm); v.y = epi_resid_mask(v.y, __uint_as_float(x.y), rm);
            v.z = epi_resid_mask(v.z, __uint_as_float(x.z), rm); v.w = epi_resid_mask(v.w, __uint_as_float(x.w), rm);
        }
        if (t.of) store_b128<EFTS_AUX_STF>(u32x4{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)}, ro, vo, row0 * (unsigned)p.ldo * 4);
        if (t.ob) {
            const unsigned sb = row0 * (unsigned)p.ldob;
            if constexpr (F & EPI_PLANE_ACT) {
                if (p.plane_act) {
                    v.x = v.x > 0.f ? v.x : v.x * p.plane_slope; v.y = v.y > 0.f ? v.y : v.y * p.plane_slope;
                    v.z = v.z > 0.f ? v.z : v.z * p.plane_slope; v.w = v.w > 0.f ? v.w : v.w * p.plane_slope;
                }
            }
            if constexpr (F & EPI_FP32) {                    // the exact value
                store_b128(u32x4{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)}, rb, vb, sb);
            } else {
                float r0, r1, r2, r3, d0, d1;
                const u32x2 hi = {pack_bf16x2(v.x, v.y, &r0, &r1), pack_bf16x2(v.z, v.w, &r2, &r3)};
                __builtin_amdgcn_raw_buffer_store_b64(hi, rb, vb, sb, EFTS_AUX_STP);
                bool lo_plane = false;
                if constexpr (F & EPI_LO) lo_plane = t.obl != nullptr;
                if (p.out_split == 2 || lo_plane) {
                    const u32x2 lo = {pack_bf16x2(r0, r1, &d0, &d1), pack_bf16x2(r2, r3, &d0, &d1)};
                    if (p.out_split == 2) __builtin_amdgcn_raw_buffer_store_b64(lo, rb, vb + 64, sb, EFTS_AUX_STP);
                    else __builtin_amdgcn_raw_buffer_store_b64(lo, rbl, vb, sb, EFTS_AUX_STP);
                }
            }
        }
    }
    return sq;
}

// The scalar fall-back sweep: threads with a real column that the vector sweep does not serve (unaligned rows, or n ends
// inside their four columns).  Element by element, plain stores, rows and columns predicated.
template <int COLS, int RPP, int NPS, unsigned F, class RowOf>
__device__ __forceinline__ void epi_sweep_scalar(const GemmKernelArgs& p, const EpiTile& t, const float* cs, RowOf rowof) {
    const int osp = (F & EPI_FP32) ? EFTS_SPLIT_FP32 : (p.out_split == 2 ? 2 : 1);
    for (int ps = 0; ps < NPS; ++ps) {
        const int trl = rowof(ps) + (int)t.trow;
        const int row = t.m0 + trl;
        if (trl >= t.bm || row >= p.m) continue;
        const float4 v = *(const float4*)(cs + (ps * RPP + t.trow) * COLS + t.c4);
        const float rm = t.rowmask ? t.rowmask[row] : 1.f;
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (t.col + u >= p.n) break;
            float x = vv[u];
            if (t.resid) x += t.resid[(long)row * p.ldr + t.col + u];
            x *= rm;
            if (t.of) t.of[(long)row * p.ldo + t.col + u] = x;
            if (t.ob) {
                if constexpr (F & EPI_PLANE_ACT) {
                    if (p.plane_act) x = x > 0.f ? x : x * p.plane_slope;
                }
                char* d = t.ob + (long)row * p.ldob + plane_off_hi(t.col + u, osp);
                if constexpr (F & EPI_FP32) {
                    *(float*)d = x;
                } else {
                    const unsigned short hi = f32_to_bf16(x);
                    *(unsigned short*)d = hi;
                    if (p.out_split == 2) *(unsigned short*)(d + 64) = f32_to_bf16(x - bf16_to_f32(hi));
                    else if constexpr (F & EPI_LO) {
                        if (t.obl) *(unsigned short*)(t.obl + (long)row * p.ldob + (t.col + u) * 2) = f32_to_bf16(x - bf16_to_f32(hi));
                    }
                }
            }
        }
    }
}

}  // namespace efts
