// efts_fft.h -- the fp32 1024-point FFT building blocks shared by the log-mel front-end (efts_frontend.hip) and the Griffin-Lim
// vocoder (efts_griffinlim.hip): complex arithmetic on register pairs, 4- and 16-point DFTs in registers, the DPP exchange inside
// a quad, the twiddle tables, and the whole transform of one wave (16 complex values per lane, one transpose through LDS).
// Behind it the same scheme for 256, 512 and 2048 points (efts_stft.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace efts {
namespace fft {

// a complex value = one register pair: +, - and the two halves of a complex product are single packed instructions (v_pk_add_f32 /
// v_pk_mul_f32 / v_pk_fma_f32 with op_sel picking the halves).  With a plain struct of two floats the vectoriser paired unrelated scalars
// and spent a fifth of the loop on v_mov to assemble the pairs.
typedef float cf __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cf cmul(cf a, cf b) { const cf bp = {-b.y, b.x}; return a.xx * b + a.yy * bp; }
__device__ __forceinline__ cf mul_mi(cf a) { const cf r = {a.y, -a.x}; return r; }                 // a * (-i)

// forward 4-point DFT in place (W4 = -i)
__device__ __forceinline__ void dft4(cf& a, cf& b, cf& c, cf& d) {
    const cf t0 = a + c, t1 = a - c, t2 = b + d, t3 = mul_mi(b - d);
    a = t0 + t2; b = t1 + t3; c = t0 - t2; d = t1 - t3;
}

// forward 16-point DFT in place, natural order in and out: n = 4 a + b, k = c + 4 d
__device__ __forceinline__ void dft16(cf* v) {
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, H = 0.70710678118654752f;
#pragma unroll
    for (int b = 0; b < 4; ++b) dft4(v[b], v[4 + b], v[8 + b], v[12 + b]);          // over a: v[4 c + b] = y_b[c]
    // y_b[c] *= W16^(b c)
    v[4 + 1] = cmul(v[4 + 1], cf{C1, -S1});  v[4 + 2] = cmul(v[4 + 2], cf{H, -H});     v[4 + 3] = cmul(v[4 + 3], cf{S1, -C1});
    v[8 + 1] = cmul(v[8 + 1], cf{H, -H});    v[8 + 2] = mul_mi(v[8 + 2]);            v[8 + 3] = cmul(v[8 + 3], cf{-H, -H});
    v[12 + 1] = cmul(v[12 + 1], cf{S1, -C1}); v[12 + 2] = cmul(v[12 + 2], cf{-H, -H}); v[12 + 3] = cmul(v[12 + 3], cf{-C1, S1});
#pragma unroll
    for (int c = 0; c < 4; ++c) dft4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);   // over b: v[4 c + d] = X[c + 4 d]
    // to natural order: X[k] sits at v[4 (k & 3) + (k >> 2)] -- a 4 x 4 transpose of the register names
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = c + 1; d < 4; ++d) { const cf t = v[4 * c + d]; v[4 * c + d] = v[4 * d + c]; v[4 * d + c] = t; }
}

template <int CTRL>
__device__ __forceinline__ cf quad(cf a) {       // the value of the quad's lane selected by the DPP quad_perm control
    cf r;
    r.x = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a.x), CTRL, 0xf, 0xf, false));
    r.y = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a.y), CTRL, 0xf, 0xf, false));
    return r;
}

// The twiddle tables of the 1024 = 16 x (16 x 4) transform, filled by the whole block of NTHREADS threads (the caller puts a barrier behind it):
// tw1s[k - 1][n2] = W1024^(n2 k), k = 1 .. 15; tw2s[q][s] = W64^(q s).
constexpr int PITCH = 68;                       // complex values per row of a wave's transpose buffer [16][PITCH]
template <int NTHREADS>
__device__ __forceinline__ void fill_twiddles(cf (*tw1s)[64], cf (*tw2s)[16]) {
    for (int i = threadIdx.x; i < 15 * 64; i += NTHREADS) {
        const int k = i / 64 + 1, n2 = i & 63;
        float sn, cs;
        sincospif(-(float)((n2 * k) & 1023) / 512.f, &sn, &cs);
        tw1s[k - 1][n2] = cf{cs, sn};
    }
    if (threadIdx.x < 64) {
        const int qq = threadIdx.x >> 4, ss = threadIdx.x & 15;
        float sn, cs;
        sincospif(-(float)((qq * ss) & 63) / 32.f, &sn, &cs);
        tw2s[qq][ss] = cf{cs, sn};
    }
}

// where bin f of a finished transform lies in the wave's buffer (the four lanes of a quad hold the same k1: without the shift
// their stores meet in the same banks)
__device__ __forceinline__ int bin_slot(int f) { return f + 4 * (f >> 8); }

// Forward 1024-point FFT of one wave.  In: v[n1] = z[64 n1 + lane], n1 = 0 .. 15.  Out: Z[f] at zw[bin_slot(f)], all LDS traffic of
// the wave retired.  zw: the wave's own [16][PITCH] buffer (nobody else reads or writes it; v is clobbered).
//   n = 64 n1 + n2, k = k1 + 16 k2:  X[k] = sum_n2 W1024^(n2 k1) W64^(n2 k2) [sum_n1 z[64 n1 + n2] W16^(n1 k1)]
//   (1) 16-point DFT over n1 in registers, twiddles W1024^(n2 k1); (2) transpose through LDS; (3) lane (k1, q) holds n2 = 4 r + q:
//   16-point DFT over r, twiddles W64^(q s), the last radix 4 across the four lanes of a quad; (4) natural order through LDS.
__device__ __forceinline__ void fft1024(cf (&v)[16], cf* zw, const cf (*tw1s)[64], const cf (*tw2s)[16], int lane) {
    const int k1 = lane >> 2, q = lane & 3;
    const float s1 = (q & 2) ? -1.f : 1.f, s2 = (q & 1) ? -1.f : 1.f;     // signs of the quad radix-4: r = partner + s * own
    dft16(v);
#pragma unroll
    for (int k = 1; k < 16; ++k) v[k] = cmul(v[k], tw1s[k - 1][lane]);
#pragma unroll
    for (int k = 0; k < 16; ++k) zw[k * PITCH + lane] = v[k];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = zw[k1 * PITCH + 4 * r + q];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    dft16(v);
#pragma unroll
    for (int s = 1; s < 16; ++s) v[s] = cmul(v[s], tw2s[q][s]);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        cf c = v[s];
        const cf p = quad<0x4E>(c);                             // quad_perm [2, 3, 0, 1]
        c = c * s1 + p;                                          // q0: x0 + x2, q1: x1 + x3, q2: x0 - x2, q3: x1 - x3
        if (q == 3) c = mul_mi(c);
        const cf p2 = quad<0xB1>(c);                            // quad_perm [1, 0, 3, 2]
        v[s] = c * s2 + p2;                                      // q0: X0, q1: X2, q2: X1, q3: X3
    }
    const int u = ((q & 1) << 1) | (q >> 1);
#pragma unroll
    for (int s = 0; s < 16; ++s) zw[k1 + 16 * s + 260 * u] = v[s];        // f = k1 + 16 s + 256 u at bin_slot(f)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---- the other sizes (efts_stft.hip): N = M x G, G = M x P lanes per transform, M complex values per lane
//   256 = 16 x 16 (P = 1, four transforms per wave), 512 = 16 x 32 (P = 2, two per wave), 2048 = 32 x 64 (P = 2, one per wave);
//   1024 = 16 x 64 (P = 4) is fft1024 above, which is this scheme written out.
//   n = G n1 + n2, k = k1 + M k2, k2 = s + M u:  W_N^(n k) = W_M^(n1 k1) W_N^(n2 k1) W_G^(n2 k2), and with n2 = P r + q
//   W_G^(n2 k2) = W_M^(r s) W_G^(q s) W_P^(q u):
//   (1) M-point DFT over n1 in registers, twiddles W_N^(n2 k1); (2) transpose through the group's LDS buffer [M][G + P];
//   (3) lane l = P k1 + q holds n2 = P r + q: M-point DFT over r, twiddles W_G^(q s), the last radix P across neighbouring lanes
//   (DPP); (4) Z[f], f = k1 + M s + M^2 u, in natural order at zw[slot(f)].

// forward 32-point DFT in place, natural order in and out: decimation in time over two 16-point DFTs
__device__ __forceinline__ void dft32(cf* v) {
    constexpr float C[16] = {1.f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f, 0.70710678118654752f, 0.55557023301960218f,
                             0.38268343236508977f, 0.19509032201612825f, 0.f, -0.19509032201612825f, -0.38268343236508977f,
                             -0.55557023301960218f, -0.70710678118654752f, -0.83146961230254524f, -0.92387953251128674f, -0.98078528040323043f};
    constexpr float S[16] = {0.f, 0.19509032201612825f, 0.38268343236508977f, 0.55557023301960218f, 0.70710678118654752f, 0.83146961230254524f,
                             0.92387953251128674f, 0.98078528040323043f, 1.f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f,
                             0.70710678118654752f, 0.55557023301960218f, 0.38268343236508977f, 0.19509032201612825f};
    cf e[16], o[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { e[i] = v[2 * i]; o[i] = v[2 * i + 1]; }
    dft16(e);
    dft16(o);
    v[0] = e[0] + o[0];
    v[16] = e[0] - o[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        const cf t = cmul(o[k], cf{C[k], -S[k]});                  // W32^k
        v[k] = e[k] + t;
        v[k + 16] = e[k] - t;
    }
}

template <int M> __device__ __forceinline__ void dftm(cf* v) {
    static_assert(M == 16 || M == 32, "16 or 32 values per lane");
    if (M == 16) dft16(v); else dft32(v);
}

template <int M, int P> struct plan {
    static_assert(P == 1 || P == 2, "the radix across lanes: none or 2 (4: fft1024)");
    static constexpr int G = M * P, N = M * G, PITCH = G + P;      // the transposed reads of step 3 then spread over all banks
    static constexpr int BUF = M * PITCH;                          // complex values of one transform's buffer
    // the P lanes that hold the same k1 store bins M^2 apart: the shift keeps them out of each other's banks
    __device__ static __forceinline__ int slot(int f) { return P == 1 ? f : f + 16 * (f / (M * M)); }
};

// tw1s[k - 1][n2] = W_N^(n2 k), k = 1 .. M - 1; tw2s[q][s] = W_G^(q s).  Filled by the whole block (the caller puts a barrier behind it).
template <int M, int P, int NTHREADS>
__device__ __forceinline__ void fill_twiddles_mp(cf (*tw1s)[M * P], cf (*tw2s)[M]) {
    constexpr int G = M * P, N = M * G;
    for (int i = threadIdx.x; i < (M - 1) * G; i += NTHREADS) {
        const int k = i / G + 1, n2 = i % G;
        float sn, cs;
        sincospif(-(float)((n2 * k) & (N - 1)) / (float)(N / 2), &sn, &cs);
        tw1s[k - 1][n2] = cf{cs, sn};
    }
    for (int i = threadIdx.x; i < P * M; i += NTHREADS) {
        const int qq = i / M, ss = i % M;
        float sn, cs;
        sincospif(-(float)((qq * ss) & (G - 1)) / (float)(G / 2), &sn, &cs);
        tw2s[qq][ss] = cf{cs, sn};
    }
}

// Forward N-point FFT of one group of G lanes.  In: v[n1] = z[G n1 + l], n1 = 0 .. M - 1, l the lane's index in its group.  Out: Z[f] at
// zw[plan::slot(f)], all LDS traffic retired.  zw: the group's own buffer of plan::BUF values; v is clobbered.
template <int M, int P>
__device__ __forceinline__ void fft_group(cf (&v)[M], cf* zw, const cf (*tw1s)[M * P], const cf (*tw2s)[M], int l) {
    typedef plan<M, P> pl;
    const int k1 = l / P, q = l % P;
    dftm<M>(v);
#pragma unroll
    for (int k = 1; k < M; ++k) v[k] = cmul(v[k], tw1s[k - 1][l]);
#pragma unroll
    for (int k = 0; k < M; ++k) zw[k * pl::PITCH + l] = v[k];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int r = 0; r < M; ++r) v[r] = zw[k1 * pl::PITCH + P * r + q];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    dftm<M>(v);
    if (P == 2) {
        const float sg = q ? -1.f : 1.f;
#pragma unroll
        for (int s = 0; s < M; ++s) {
            const cf c = s ? cmul(v[s], tw2s[q][s]) : v[s];
            const cf p = quad<0xB1>(c);                             // quad_perm [1, 0, 3, 2]
            v[s] = c * sg + p;                                       // q0: x0 + x1 = X0, q1: x0 - x1 = X1
        }
    }
#pragma unroll
    for (int s = 0; s < M; ++s) zw[pl::slot(k1 + M * s + M * M * q)] = v[s];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

}  // namespace fft
}  // namespace efts
