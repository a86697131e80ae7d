// efts_snake.hip -- BigVGAN's anti-aliased periodic activation (Activation1d around Snake / SnakeBeta) as one launch: upsample by 2 with a
// 12-tap Kaiser sinc, v = u + inv_b sin(a u)^2 per channel, low-pass and downsample by 2 with the same filter, replicate padding at each
// item's ends.  include/efts_abi.h has the definition to the order of every sum; DESIGN.md the numbers.
//
// Channel-last fp32 rows in, an operand plane and / or fp32 rows out.  One lane owns 4 adjacent channels (16-byte loads and stores,
// coalesced across the lanes of a row) and EFTS_SNAKE_SEG consecutive rows of one item.  It walks down its rows with two windows in
// registers: the 6 rows of x that one PAIR of 2x-rate samples needs, and the 12 values of v that one output row needs.
//   pair p = (v(2p + 1), v(2p + 2)), both from X(p - 2 .. p + 3); row t reads the pairs t - 3 .. t + 2, i.e. x[t - 5 .. t + 5].
//   The clamp of the 2x-rate index to 0 .. 2L - 1 turns into a clamp of the pair index to -1 .. L - 1: pair -1 is (v(0), v(0)), pair L - 1
//   is (v(2L - 1), v(2L - 1)), and every pair outside repeats those.
// A segment starts by computing the 5 pairs in front of its first row again (10 of 12 values, from 10 rows of halo): no LDS, no barrier,
// no dependence on where a segment begins.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_internal.h"

namespace {

using namespace efts;

// f[0..5] of the definition (f[11 - k] = f[k]): float64 values, rounded once
#define SNAKE_F0 0.0020289664498962423f
#define SNAKE_F1 0.00938946394406788f
#define SNAKE_F2 (-0.02554346406529466f)
#define SNAKE_F3 (-0.05765737547536495f)
#define SNAKE_F4 0.12857260908132875f
#define SNAKE_F5 0.4432098000653667f

struct SnakeArgs {
    const float* x; const int* lengths; const float* a; const float* inv_b; char* plane; float* out;
    long ldx, ldp, ldo;
    int split, pitch, rows_item, T, len_mul, c, kp;
};

__device__ __forceinline__ float snake_sin(float t) {
#ifdef EFTS_SNAKE_FAST_SIN
    return __sinf(t);            // (experiments only: the shipped library calls sinf)
#else
    return sinf(t);
#endif
}

// u = 2 * sum_i f_i X_i in ascending i by fma, then v = fma(inv_b, s * s, u) with s = sin(a * u)
__device__ __forceinline__ float snake_v(float f0, float f1, float f2, float f3, float f4, float f5, float x0, float x1, float x2, float x3,
                                         float x4, float x5, float a, float inv_b) {
    float acc = 0.f;
    acc = fmaf(f0, x0, acc); acc = fmaf(f1, x1, acc); acc = fmaf(f2, x2, acc);
    acc = fmaf(f3, x3, acc); acc = fmaf(f4, x4, acc); acc = fmaf(f5, x5, acc);
    const float u = 2.f * acc;
    const float s = snake_sin(a * u);
    return fmaf(inv_b, s * s, u);
}

__device__ __forceinline__ void snake_store(const SnakeArgs& p, long row, int c4, int last_quad, float4 y) {
    if (p.out) *(float4*)(p.out + row * p.ldo + c4) = y;
    if (p.plane) {
        char* prow = p.plane + row * p.ldp;
        plane_store4(prow, c4, y.x, y.y, y.z, y.w, p.split);
        if (last_quad)                                   // the padding columns of the last chunk
            for (int k = p.c; k < p.kp; k += 4) plane_store4(prow, k, 0.f, 0.f, 0.f, 0.f, p.split);
    }
}

__global__ __launch_bounds__(256) void snake_aa_kernel(SnakeArgs p) {
    const int q = p.c >> 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int nseg = (p.rows_item + EFTS_SNAKE_SEG - 1) / EFTS_SNAKE_SEG;
    if (idx >= (long)nseg * q) return;
    const int seg = (int)(idx / q), cq = (int)(idx - (long)seg * q), c4 = cq << 2, b = blockIdx.y;
    const int last_quad = cq == q - 1;
    const int t0 = seg * EFTS_SNAKE_SEG;
    const int t1 = t0 + EFTS_SNAKE_SEG < p.rows_item ? t0 + EFTS_SNAKE_SEG : p.rows_item;
    int L = p.lengths[b];
    L = L < 0 ? 0 : L > p.T ? p.T : L;
    L *= p.len_mul;                                      // (T * len_mul = rows_item <= pitch fits an int: checked by the host)
    const long row0 = (long)b * p.pitch;
    const int live = t1 < L ? t1 : L;                    // rows t0 .. live - 1 are computed, live .. t1 - 1 are zero

    if (t0 < L) {
        const float4 a = *(const float4*)(p.a + c4), ib = *(const float4*)(p.inv_b + c4);
        const float* const xb = p.x + row0 * p.ldx + c4;
        auto X = [&](int r) -> float4 {                  // X(r) = x[clamp(r, 0, L - 1)]
            r = r < 0 ? 0 : r > L - 1 ? L - 1 : r;
            return *(const float4*)(xb + (long)r * p.ldx);
        };
        float4 xw[6];                                    // X(pe - 2 .. pe + 3) of the current pair
        float4 vw[12];                                   // v(2t - 5 .. 2t + 6) once pair t + 2 is in
        float4 vo, ve;
        int pe_prev = -8;                                // (no pair: pe >= -1)
#pragma unroll
        for (int k = 0; k < 12; ++k) vw[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int pr = t0 - 3; pr <= live + 1; ++pr) {
            const int pe = pr < -1 ? -1 : pr > L - 1 ? L - 1 : pr;
            if (pe != pe_prev) {
                if (pe == pe_prev + 1) {
#pragma unroll
                    for (int k = 0; k < 5; ++k) xw[k] = xw[k + 1];
                    xw[5] = X(pe + 3);
                } else {                                 // the first pair of the segment
#pragma unroll
                    for (int k = 0; k < 6; ++k) xw[k] = X(pe - 2 + k);
                }
                pe_prev = pe;
                // odd sample 2 pe + 1: taps f[0], f[2], .. on X(pe + 3), X(pe + 2), ..; even sample 2 pe + 2: taps f[1], f[3], .. on the same rows
                // (f[6 .. 11] = f[5 .. 0])
                vo.x = snake_v(SNAKE_F0, SNAKE_F2, SNAKE_F4, SNAKE_F5, SNAKE_F3, SNAKE_F1, xw[5].x, xw[4].x, xw[3].x, xw[2].x, xw[1].x, xw[0].x, a.x, ib.x);
                vo.y = snake_v(SNAKE_F0, SNAKE_F2, SNAKE_F4, SNAKE_F5, SNAKE_F3, SNAKE_F1, xw[5].y, xw[4].y, xw[3].y, xw[2].y, xw[1].y, xw[0].y, a.y, ib.y);
                vo.z = snake_v(SNAKE_F0, SNAKE_F2, SNAKE_F4, SNAKE_F5, SNAKE_F3, SNAKE_F1, xw[5].z, xw[4].z, xw[3].z, xw[2].z, xw[1].z, xw[0].z, a.z, ib.z);
                vo.w = snake_v(SNAKE_F0, SNAKE_F2, SNAKE_F4, SNAKE_F5, SNAKE_F3, SNAKE_F1, xw[5].w, xw[4].w, xw[3].w, xw[2].w, xw[1].w, xw[0].w, a.w, ib.w);
                ve.x = snake_v(SNAKE_F1, SNAKE_F3, SNAKE_F5, SNAKE_F4, SNAKE_F2, SNAKE_F0, xw[5].x, xw[4].x, xw[3].x, xw[2].x, xw[1].x, xw[0].x, a.x, ib.x);
                ve.y = snake_v(SNAKE_F1, SNAKE_F3, SNAKE_F5, SNAKE_F4, SNAKE_F2, SNAKE_F0, xw[5].y, xw[4].y, xw[3].y, xw[2].y, xw[1].y, xw[0].y, a.y, ib.y);
                ve.z = snake_v(SNAKE_F1, SNAKE_F3, SNAKE_F5, SNAKE_F4, SNAKE_F2, SNAKE_F0, xw[5].z, xw[4].z, xw[3].z, xw[2].z, xw[1].z, xw[0].z, a.z, ib.z);
                ve.w = snake_v(SNAKE_F1, SNAKE_F3, SNAKE_F5, SNAKE_F4, SNAKE_F2, SNAKE_F0, xw[5].w, xw[4].w, xw[3].w, xw[2].w, xw[1].w, xw[0].w, a.w, ib.w);
                if (pe == -1) vo = ve;                   // 2 pe + 1 = -1 clamps to sample 0
                if (pe == L - 1) ve = vo;                // 2 pe + 2 = 2L clamps to sample 2L - 1
            }
#pragma unroll
            for (int k = 0; k < 10; ++k) vw[k] = vw[k + 2];
            vw[10] = vo;
            vw[11] = ve;
            const int t = pr - 2;
            if (t >= t0) {
                float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
#define SNAKE_TAP(K, F) y.x = fmaf(F, vw[K].x, y.x); y.y = fmaf(F, vw[K].y, y.y); y.z = fmaf(F, vw[K].z, y.z); y.w = fmaf(F, vw[K].w, y.w);
                SNAKE_TAP(0, SNAKE_F0) SNAKE_TAP(1, SNAKE_F1) SNAKE_TAP(2, SNAKE_F2) SNAKE_TAP(3, SNAKE_F3) SNAKE_TAP(4, SNAKE_F4) SNAKE_TAP(5, SNAKE_F5)
                SNAKE_TAP(6, SNAKE_F5) SNAKE_TAP(7, SNAKE_F4) SNAKE_TAP(8, SNAKE_F3) SNAKE_TAP(9, SNAKE_F2) SNAKE_TAP(10, SNAKE_F1) SNAKE_TAP(11, SNAKE_F0)
#undef SNAKE_TAP
                snake_store(p, row0 + t, c4, last_quad, y);
            }
        }
    }
    for (int t = live > t0 ? live : t0; t < t1; ++t) snake_store(p, row0 + t, c4, last_quad, make_float4(0.f, 0.f, 0.f, 0.f));
}

}  // namespace

extern "C" int efts_snake_aa(const efts_snake_aa_args* a, void* stream) {
    if (!a) return efts_fail(EFTS_EINVAL, "efts_snake_aa: null args");
    if (!a->x || !a->lengths || !a->a || !a->inv_b) return efts_fail(EFTS_EINVAL, "efts_snake_aa: null operand");
    if (!a->plane && !a->out) return efts_fail(EFTS_EINVAL, "efts_snake_aa: neither a plane nor an fp32 output");
    if (a->plane && !(a->split >= EFTS_SPLIT_BF16 && a->split <= EFTS_SPLIT_FP32)) return efts_fail(EFTS_EINVAL, "efts_snake_aa: split must be 1, 2 or 3");
    if (a->reserved != 0 || a->reserved2 != 0) return efts_fail(EFTS_EINVAL, "efts_snake_aa: reserved must be 0");
    if (a->c < 4 || (a->c & 3)) return efts_fail(EFTS_ESHAPE, "efts_snake_aa: c must be a positive multiple of 4");
    if (a->B < 1 || a->B > 65535) return efts_fail(EFTS_ESHAPE, "efts_snake_aa: 1 .. 65535 items per launch");
    if (a->T < 1 || a->len_mul < 1 || a->pitch < 1) return efts_fail(EFTS_ESHAPE, "efts_snake_aa: T, len_mul and pitch must be positive");
    if ((int64_t)a->T * a->len_mul > a->pitch) return efts_fail(EFTS_ESHAPE, "efts_snake_aa: T * len_mul rows above the pitch");
    if ((int64_t)a->B * a->pitch > 0x7fffffff) return efts_fail(EFTS_ESHAPE, "efts_snake_aa: B * pitch rows above 2^31 - 1");
    const int chunk = a->split == EFTS_SPLIT_BF16 ? 64 : 32, kp = (a->c + chunk - 1) / chunk * chunk;
    if (a->ldx < a->c || (a->out && a->ldo < a->c)) return efts_fail(EFTS_ESHAPE, "efts_snake_aa: a row stride below the row");
    if (a->plane && a->ld_plane < (int64_t)(kp / chunk) * 128) return efts_fail(EFTS_ESHAPE, "efts_snake_aa: ld_plane below the chunks of c columns");
    if (((uintptr_t)a->x & 15) || (a->ldx & 3) || ((uintptr_t)a->a & 15) || ((uintptr_t)a->inv_b & 15) || ((uintptr_t)a->lengths & 3))
        return efts_fail(EFTS_EALIGN, "efts_snake_aa: x, a, inv_b and the row stride of x must be 16-byte aligned, lengths 4-byte");
    if (a->out && (((uintptr_t)a->out & 15) || (a->ldo & 3))) return efts_fail(EFTS_EALIGN, "efts_snake_aa: out and its row stride must be 16-byte aligned");
    if (a->plane && (((uintptr_t)a->plane & 15) || (a->ld_plane & 15))) return efts_fail(EFTS_EALIGN, "efts_snake_aa: plane and ld_plane must be 16-byte aligned");

    SnakeArgs k;
    k.x = a->x; k.lengths = a->lengths; k.a = a->a; k.inv_b = a->inv_b; k.plane = (char*)a->plane; k.out = a->out;
    k.ldx = a->ldx; k.ldp = a->ld_plane; k.ldo = a->ldo;
    k.split = a->plane ? a->split : EFTS_SPLIT_FP32; k.pitch = a->pitch; k.rows_item = a->T * a->len_mul; k.T = a->T; k.len_mul = a->len_mul;
    k.c = a->c; k.kp = kp;
    const int64_t lanes = (int64_t)((k.rows_item + EFTS_SNAKE_SEG - 1) / EFTS_SNAKE_SEG) * (a->c >> 2);
    const dim3 grid((unsigned)((lanes + 255) / 256), a->B);
    hipLaunchKernelGGL(snake_aa_kernel, grid, dim3(256), 0, (hipStream_t)stream, k);
    return efts_check_launch("efts_snake_aa");
}
