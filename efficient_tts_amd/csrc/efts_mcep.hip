// efts_mcep.hip -- a linear map of the log power spectrum of every frame of a waveform batch, in one launch (efts_logspec_project), and the
// summed distance between the frames of two feature sequences paired one to one (efts_frame_dist).  include/efts_abi.h has the definitions;
// efficient_tts_amd/mcep.py builds the table that turns the first into order-24 all-pass-warped mel-cepstra and both into the mel-cepstral
// distortion that the TTS literature reports.  The kernel itself knows nothing about cepstra.
//
//   logspec_project_kernel : the framing, the window, the transform and the clamp of efts_stft_mag (efts_stft_frame.h, efts_fft.h; N = 1024: one
//                            wave per PAIR of neighbouring frames), then L = ln P per bin in registers and out[k] = sum_f table[k][f] L[f].
//                            No spectrum goes to memory.  The table ([n_coef][513] fp32, 49 KB at n_coef = 24, 66 KB at 32) is staged once
//                            per workgroup into LDS and read by all LP_WAVES waves for LP_ITER pairs each: 64 pairs per staging.
//                            Projection: lane l takes its bins l, l + 64, .. in ascending order by fma -- every table word is read once per
//                            pair and serves both frames --, which leaves 2 x 32 lane sums per lane.  They are summed across the wave by a
//                            TRANSPOSING tree: at distance 32 a lane keeps one half of its 64 values and hands the other half to its partner,
//                            at 16 a half of the rest, ..: 63 exchanges instead of 64 x 6, the same additions as v += (v of the lane 32, 16,
//                            .., 1 across) (fp32 + is commutative), and lane 32 j + k ends up with coefficient k of frame j: one coalesced store.
//   LDS                    : 8 transform buffers of 8.5 KB + 8 KB of twiddles = 76 KB, + the table: 124 KB at n_coef = 24, 140 KB at 32, of the
//                            160 KB of a CU.  So ONE workgroup of 8 waves per CU, two waves per SIMD; the registers (under 256) do not bind.
//   frame_dist_kernel      : one workgroup per item; d(t, t) as efts_dtw computes its local cost, added in float64 in frame order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_internal.h"
#include "efts_fft.h"
#include "efts_stft_frame.h"

namespace efts {

constexpr int LP_N = 1024, LP_BINS = LP_N / 2 + 1, LP_NB = (LP_BINS + 63) / 64;       // bins per lane: 9, the last one on lane 0 alone
constexpr int LP_WAVES = 8, LP_THREADS = 64 * LP_WAVES, LP_ITER = 8, LP_UPB = LP_WAVES * LP_ITER;      // frame pairs per workgroup
constexpr int LP_MAX_COEF = 32;
constexpr int LP_BUF = 16 * fft::PITCH;                                                 // complex values of one wave's transform buffer
constexpr size_t LP_LDS_FIXED = sizeof(fft::cf) * (LP_WAVES * LP_BUF + 15 * 64 + 4 * 16);

__global__ __launch_bounds__(LP_THREADS) void logspec_project_kernel(const void* __restrict__ audio, int pcm, float pcm_scale, long ld,
                                                                     const int* __restrict__ lengths, int max_len, const float* __restrict__ window,
                                                                     const float* __restrict__ table, int n_coef, float* __restrict__ out,
                                                                     int* __restrict__ frames, int H, int W, int T_max) {
    using namespace fft;
    extern __shared__ __attribute__((aligned(16))) cf lp_lds[];
    cf* zs = lp_lds;                                               // [LP_WAVES][LP_BUF]
    cf (*tw1s)[64] = (cf (*)[64])(zs + LP_WAVES * LP_BUF);         // [15][64]
    cf (*tw2s)[16] = (cf (*)[16])(tw1s + 15);                      // [4][16]
    float* tab = (float*)(tw2s + 4);                               // [n_coef][LP_BINS]
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = st_len(lengths, b, max_len), T = st_frames(len, LP_N, H);       // as efts_stft_mag
    const int p0 = blockIdx.x * LP_UPB;
    if (blockIdx.x == 0 && threadIdx.x == 0) frames[b] = T;
    float win[16];
    if (2 * p0 < T) {                                              // (uniform) a workgroup behind the item's frames only writes zeros
        fill_twiddles<LP_THREADS>(tw1s, tw2s);
        for (int i = threadIdx.x; i < n_coef * LP_BINS; i += LP_THREADS) tab[i] = table[i];
        __syncthreads();
        st_window_regs<16, 64>(window, W, LP_N, lane, win);
    }
    cf* zw = zs + wave * LP_BUF;
    const int fr = lane >> 5, kk = lane & 31;                      // what the lane holds after the tree: coefficient kk of frame t0 + fr
    // from here on nothing synchronises more than one wave
    for (int it = 0; it < LP_ITER; ++it) {
        const int t0 = 2 * (p0 + it * LP_WAVES + wave);
        if (t0 >= T_max) continue;
        float res = 0.f;                                           // rows at and beyond the item's count are zero
        if (t0 < T) {
            const bool vb = t0 + 1 < T;
            const int s0 = t0 * H - LP_N / 2;
            cf v[16];
            if (pcm) st_load<short, LP_N, 16, 64>((const short*)audio + (long)b * ld, pcm_scale, len, s0, H, vb, lane, win, v);
            else     st_load<float, LP_N, 16, 64>((const float*)audio + (long)b * ld, 1.f, len, s0, H, vb, lane, win, v);
            fft1024(v, zw, tw1s, tw2s, lane);
            float la[LP_NB], lb[LP_NB];
#pragma unroll
            for (int i = 0; i < LP_NB; ++i) {
                const int f = lane + 64 * i;
                la[i] = lb[i] = 0.f;
                if (f < LP_BINS) {
                    float ar, ai, br, bi;
                    st_split(zw[bin_slot(f)], zw[bin_slot((LP_N - f) & (LP_N - 1))], ar, ai, br, bi);
                    la[i] = logf(fmaxf(fmaf(ar, ar, ai * ai), 1e-7f));                  // the clamp of efts_stft_mag, before its square root
                    lb[i] = logf(fmaxf(fmaf(br, br, bi * bi), 1e-7f));
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the next transform overwrites zw
            float acc[2 * LP_MAX_COEF];
#pragma unroll
            for (int k = 0; k < LP_MAX_COEF; ++k) {
                float sa = 0.f, sb = 0.f;
                if (k < n_coef) {                                  // (uniform)
                    const float* row = tab + k * LP_BINS + lane;
#pragma unroll
                    for (int i = 0; i < LP_NB - 1; ++i) {
                        const float w = row[64 * i];
                        sa = fmaf(w, la[i], sa);
                        sb = fmaf(w, lb[i], sb);
                    }
                    if (lane == 0) {                               // bin 512
                        const float w = row[64 * (LP_NB - 1)];
                        sa = fmaf(w, la[LP_NB - 1], sa);
                        sb = fmaf(w, lb[LP_NB - 1], sb);
                    }
                }
                acc[k] = sa;
                acc[LP_MAX_COEF + k] = sb;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {                     // o values stay per lane after this step
                const bool up = (lane & o) != 0;
#pragma unroll
                for (int j = 0; j < o; ++j) {
                    const float keep = up ? acc[j + o] : acc[j], send = up ? acc[j] : acc[j + o];
                    acc[j] = keep + __shfl_xor(send, o);
                }
            }
            if (t0 + fr < T) res = acc[0];
        }
        if (kk < n_coef && t0 + fr < T_max) out[((long)b * T_max + t0 + fr) * n_coef + kk] = res;
    }
}

constexpr int FD_THREADS = 256, FD_CHUNK = 1024, FD_MAX_DIM = 32;

__global__ __launch_bounds__(FD_THREADS) void frame_dist_kernel(const float* __restrict__ x, long ldx, long x_item_stride, const int* __restrict__ x_frames, int Tx,
                                                                const float* __restrict__ y, long ldy, long y_item_stride, const int* __restrict__ y_frames, int Ty,
                                                                int D, double* __restrict__ cost, int* __restrict__ count) {
    __shared__ float ds[FD_CHUNK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = max(0, min(min(x_frames[b], Tx), min(y_frames[b], Ty)));             // (uniform) rows at and beyond n are never read
    const float* xb = x + (long)b * x_item_stride;
    const float* yb = y + (long)b * y_item_stride;
    double acc = 0.0;
    for (int c0 = 0; c0 < n; c0 += FD_CHUNK) {
        const int m = min(FD_CHUNK, n - c0);
        __syncthreads();
        for (int i = tid; i < m; i += FD_THREADS) {
            const float* xr = xb + (long)(c0 + i) * ldx;
            const float* yr = yb + (long)(c0 + i) * ldy;
            float s = 0.f;
            for (int k = 0; k < D; ++k) {                          // the local cost of efts_dtw: the fused sum of squares in ascending k
                const float d = xr[k] - yr[k];
                s = fmaf(d, d, s);
            }
            ds[i] = sqrtf(s);
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < m; ++i) acc += (double)ds[i];
    }
    if (tid == 0) {
        cost[b] = n > 0 ? acc : (double)__builtin_nanf("");
        count[b] = n;
    }
}

}  // namespace efts

using namespace efts;

extern "C" int efts_logspec_project(const void* audio, int32_t pcm16, float pcm_scale, int64_t ld, const int32_t* lengths, int32_t max_len,
                                    const float* window, const float* table, int32_t n_coef, float* out, int32_t* frames, int32_t B, int32_t N, int32_t H,
                                    int32_t W, void* stream) {
    if (N != LP_N) return efts_fail(EFTS_ESHAPE, "efts_logspec_project: the FFT size must be 1024");
    if (H < 1 || H > N) return efts_fail(EFTS_ESHAPE, "efts_logspec_project: the hop must lie in 1 .. the FFT size");
    if (W < 2 || W > N) return efts_fail(EFTS_ESHAPE, "efts_logspec_project: the window length must lie in 2 .. the FFT size");
    if (n_coef < 1 || n_coef > LP_MAX_COEF) return efts_fail(EFTS_ESHAPE, "efts_logspec_project: n_coef 1 .. %d", LP_MAX_COEF);
    if (const char* why = efts_audio_bad_shape(B, max_len)) return efts_fail(EFTS_ESHAPE, "efts_logspec_project: %s", why);
    if (ld < max_len) return efts_fail(EFTS_ESHAPE, "efts_logspec_project: the leading dimension is smaller than the longest item");
    if (!audio || !lengths || !window || !table || !out || !frames) return efts_fail(EFTS_EINVAL, "efts_logspec_project: null pointer");
    if (((uintptr_t)audio % (pcm16 ? 2 : 4)) || ((uintptr_t)lengths & 3) || ((uintptr_t)window & 3) || ((uintptr_t)table & 3) || ((uintptr_t)out & 3) ||
        ((uintptr_t)frames & 3))
        return efts_fail(EFTS_EINVAL, "efts_logspec_project: a pointer is not aligned to its element");
    const int T_max = 1 + max_len / H;
    const size_t lds = LP_LDS_FIXED + sizeof(float) * (size_t)n_coef * LP_BINS;
    // more than 64 KiB of dynamic LDS is an opt-in: asked for once, for the largest table (a host-side attribute, no launch)
    static bool attr = false;
    if (!attr) {
        const size_t most = LP_LDS_FIXED + sizeof(float) * (size_t)LP_MAX_COEF * LP_BINS;
        const hipError_t e = hipFuncSetAttribute((const void*)logspec_project_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
        if (e != hipSuccess) return efts_fail(EFTS_ELAUNCH, "efts_logspec_project: %zu bytes of LDS refused: %s", most, hipGetErrorString(e));
        attr = true;
    }
    const unsigned pairs = (unsigned)((T_max + 1) / 2);
    hipLaunchKernelGGL(logspec_project_kernel, dim3((pairs + LP_UPB - 1) / LP_UPB, (unsigned)B), dim3(LP_THREADS), lds, (hipStream_t)stream, audio, pcm16,
                       pcm_scale, (long)ld, lengths, max_len, window, table, n_coef, out, frames, H, W, T_max);
    return efts_check_launch("efts_logspec_project");
}

extern "C" int efts_frame_dist(const float* x, int64_t ldx, int64_t x_item_stride, const int32_t* x_frames, int32_t Tx, const float* y, int64_t ldy,
                               int64_t y_item_stride, const int32_t* y_frames, int32_t Ty, int32_t D, double* cost, int32_t* count, int32_t B, void* stream) {
    if (D < 1 || D > FD_MAX_DIM) return efts_fail(EFTS_ESHAPE, "efts_frame_dist: D 1 .. %d", FD_MAX_DIM);
    if (B < 1 || B > 65535 || Tx < 1 || Ty < 1 || ldx < D || ldy < D || x_item_stride < 0 || y_item_stride < 0)
        return efts_fail(EFTS_ESHAPE, "efts_frame_dist: 1 .. 65535 items, Tx and Ty >= 1, row strides >= D, item strides >= 0");
    if (!x || !x_frames || !y || !y_frames || !cost || !count) return efts_fail(EFTS_EINVAL, "efts_frame_dist: null pointer");
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)x_frames & 3) || ((uintptr_t)y_frames & 3) || ((uintptr_t)cost & 7) || ((uintptr_t)count & 3))
        return efts_fail(EFTS_EINVAL, "efts_frame_dist: a pointer is not aligned to its element");
    hipLaunchKernelGGL(frame_dist_kernel, dim3((unsigned)B), dim3(FD_THREADS), 0, (hipStream_t)stream, x, (long)ldx, (long)x_item_stride, x_frames, Tx, y, (long)ldy,
                       (long)y_item_stride, y_frames, Ty, D, cost, count);
    return efts_check_launch("efts_frame_dist");
}
