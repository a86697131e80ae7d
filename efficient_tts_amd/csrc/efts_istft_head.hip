// efts_istft_head.hip -- the head of an iSTFTNet generator: the fp32 output of conv_post, N + 2 channels per frame (a log-magnitude and a
// phase argument per bin), to audio by an N-point inverse real DFT, the periodic Hann window and an overlap-add with hop h = N / 4 divided
// by the true window envelope.  include/efts_abi.h has the definition to the bit; DESIGN.md the numbers.
//
// A workgroup (256 lanes) owns EFTS_ISTFT_RUN = 1024 consecutive samples of one item, FR = 1024 / h hops q0 .. q0 + FR - 1.  Sample
// t = h q + r is touched by the frames q - 1 .. q + 2, so the run needs the frames q0 - 1 .. q0 + FR + 1, clipped to the item's 0 .. L:
//   1. frames q0 - 2 .. of z (an even first row: (N + 2) * 4 bytes per row is 8 mod 16) go to LDS by 16-byte loads; what lies outside
//      z is not read, what lies outside the item's frames is never used;
//   2. one lane per (frame, bin): exp, sin, sincos -> Re X, Im X, in place;
//   3. one lane per (frame, n): the inverse real DFT from the twiddle table at (k n) mod N, times the window, into a second LDS tile;
//   4. one lane per four consecutive samples: the at most four frames in ascending order, the envelope from the window table, one
//      16-byte store.
// The second kernel copies one row of an operand plane per item (the reflected row in front of the item, see the header).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "efts_internal.h"

namespace {

struct HeadArgs {
    const float* z; const int* lengths; const float* window; const float* twiddle; float* audio;
    long ld_audio;
    int pitch, z_rows, len_mul, out_len;
};

template <int N>
__global__ __launch_bounds__(256) void istft_head_kernel(HeadArgs p) {
    constexpr int H = N / 4, K = N / 2 + 1, C = N + 2;
    constexpr int FR = EFTS_ISTFT_RUN / H;           // hops per run
    constexpr int NF = FR + 4;                       // staged frames: q0 - 2 .. q0 + FR + 1
    constexpr int NP = N + 4;                        // row stride of the windowed frames (padded: a lane's 16-byte reads spread over the banks)
    __shared__ __attribute__((aligned(16))) float zs[NF * C];
    __shared__ __attribute__((aligned(16))) float wy[(FR + 3) * NP];
    __shared__ float tw[2 * N];
    __shared__ float win[N];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int q0 = blockIdx.x * FR;
    const int t0 = blockIdx.x * EFTS_ISTFT_RUN + 4 * tid;
    float* const dst = p.audio + (long)b * p.ld_audio + t0;

    int L = p.lengths[b];
    L = L < 0 ? 0 : L;
    {
        const long rows = (long)L * p.len_mul;
        const int cap = p.out_len / H < p.pitch - 1 ? p.out_len / H : p.pitch - 1;
        L = rows < cap ? (int)rows : cap;
    }
    if (q0 >= L) {                                   // (uniform over the workgroup) the run lies behind the item: silence
        if (t0 < p.out_len) *(float4*)dst = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int fa = q0 > 0 ? q0 - 1 : 0;              // frames of the item that touch the run
    const int fb = q0 + FR + 1 < L ? q0 + FR + 1 : L;

    if (tid < 2 * N) tw[tid] = p.twiddle[tid];
    if (tid < N) win[tid] = p.window[tid];
    // ---- 1. z rows b * pitch + q0 - 2 .. b * pitch + fb
    {
        const long base = ((long)b * p.pitch + q0 - 2) * C, total = (long)p.z_rows * C;
        const int pieces = ((fb - (q0 - 2) + 1) * C + 3) >> 2;
        for (int i = tid; i < pieces; i += 256) {
            const long o = base + 4 * i;
            float4 v;
            if (o >= 0 && o + 4 <= total) {
                v = *(const float4*)(p.z + o);
            } else {
                v.x = (o >= 0 && o < total) ? p.z[o] : 0.f;
                v.y = (o + 1 >= 0 && o + 1 < total) ? p.z[o + 1] : 0.f;
                v.z = (o + 2 >= 0 && o + 2 < total) ? p.z[o + 2] : 0.f;
                v.w = (o + 3 >= 0 && o + 3 < total) ? p.z[o + 3] : 0.f;
            }
            *(float4*)(zs + 4 * i) = v;              // (pieces * 4 <= NF * C: fb <= q0 + FR + 1)
        }
    }
    __syncthreads();
    // ---- 2. the spectrum, in place
    const int nfr = fb - fa + 1;
    for (int i = tid; i < nfr * K; i += 256) {
        const int f = i / K, k = i - f * K;
        float* row = zs + (fa - (q0 - 2) + f) * C;
        const float mag = expf(row[k]), ph = sinf(row[K + k]);
        float s, c;
        sincosf(ph, &s, &c);
        row[k] = mag * c;
        row[K + k] = mag * s;
    }
    __syncthreads();
    // ---- 3. w[n] * y_f[n]
    for (int i = tid; i < nfr * N; i += 256) {
        const int f = i / N, n = i - f * N;
        const float* row = zs + (fa - (q0 - 2) + f) * C;
        float acc = 0.f;
#pragma unroll
        for (int k = 1; k < N / 2; ++k) {
            const int j = (k * n) & (N - 1);
            acc = fmaf(row[k], tw[2 * j], acc);
            acc = fmaf(-row[K + k], tw[2 * j + 1], acc);
        }
        const float dc = row[0] + ((n & 1) ? -row[N / 2] : row[N / 2]);
        const float y = (dc + 2.f * acc) * (1.f / N);
        wy[(fa - (q0 - 1) + f) * NP + n] = win[n] * y;
    }
    __syncthreads();
    // ---- 4. overlap-add
    if (t0 >= p.out_len) return;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tl = 4 * tid + j;                  // sample of the run
        const int ql = tl / H, r = tl - ql * H;      // hop of the run; frame q0 + ql - 1 + i holds the sample at r + (3 - i) * H
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = q0 + ql - 1 + i, n = r + (3 - i) * H;
            if (f >= 0 && f <= L) {
                num += wy[(ql + i) * NP + n];
                den += win[n] * win[n];
            }
        }
        o[j] = q0 + ql < L ? num / den : 0.f;
    }
    *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
}

// row b * pitch + 1 of the plane -> row b * pitch - 1, 16 bytes per lane
__global__ __launch_bounds__(256) void istft_reflect_kernel(char* plane, long ld, int pitch) {
    const char* src = plane + ((long)blockIdx.x * pitch + 1) * ld;
    char* dst = plane + ((long)blockIdx.x * pitch - 1) * ld;
    for (long o = (long)threadIdx.x * 16; o < ld; o += 256 * 16) *(uint4*)(dst + o) = *(const uint4*)(src + o);
}

}  // namespace

extern "C" int efts_istft_head(const efts_istft_head_args* a, void* stream) {
    if (!a) return efts_fail(EFTS_EINVAL, "efts_istft_head: null args");
    if (a->mode != EFTS_ISTFT_SYNTH && a->mode != EFTS_ISTFT_REFLECT) return efts_fail(EFTS_EINVAL, "efts_istft_head: mode must be 0 (synthesis) or 1 (reflected row)");
    if (a->reserved != 0 || a->reserved2 != 0) return efts_fail(EFTS_EINVAL, "efts_istft_head: reserved must be 0");
    if (a->B < 1 || a->B > 65535) return efts_fail(EFTS_ESHAPE, "efts_istft_head: 1 .. 65535 items per launch");
    if (a->pitch < 4 || (a->pitch & 1)) return efts_fail(EFTS_ESHAPE, "efts_istft_head: pitch must be even and at least 4 rows");
    hipStream_t st = (hipStream_t)stream;
    if (a->mode == EFTS_ISTFT_REFLECT) {
        if (!a->plane) return efts_fail(EFTS_EINVAL, "efts_istft_head: null plane");
        if (a->ld_plane < 16) return efts_fail(EFTS_ESHAPE, "efts_istft_head: ld_plane below one 16-byte piece");
        if (((uintptr_t)a->plane & 15) || (a->ld_plane & 15)) return efts_fail(EFTS_EALIGN, "efts_istft_head: plane and ld_plane must be 16-byte aligned");
        hipLaunchKernelGGL(istft_reflect_kernel, dim3(a->B), dim3(256), 0, st, (char*)a->plane, (long)a->ld_plane, a->pitch);
        return efts_check_launch("efts_istft_head");
    }
    if (!(a->n_fft == 8 || a->n_fft == 16 || a->n_fft == 32)) return efts_fail(EFTS_EINVAL, "efts_istft_head: n_fft must be 8, 16 or 32");
    if (a->hop * 4 != a->n_fft) return efts_fail(EFTS_EINVAL, "efts_istft_head: hop must be n_fft / 4");
    if (!a->z || !a->lengths || !a->window || !a->twiddle || !a->audio) return efts_fail(EFTS_EINVAL, "efts_istft_head: null operand");
    if (a->len_mul < 1 || a->z_rows < 1) return efts_fail(EFTS_ESHAPE, "efts_istft_head: len_mul and z_rows must be positive");
    if (a->out_len < 4 || (a->out_len & 3) || a->out_len > 0x7fffffff - 4 * EFTS_ISTFT_RUN) return efts_fail(EFTS_ESHAPE, "efts_istft_head: out_len must be a multiple of 4 in 4 .. 2^31 - 4097");
    if (a->ld_audio < a->out_len) return efts_fail(EFTS_ESHAPE, "efts_istft_head: ld_audio below out_len");
    if (((uintptr_t)a->z & 15) || ((uintptr_t)a->audio & 15) || (a->ld_audio & 3))
        return efts_fail(EFTS_EALIGN, "efts_istft_head: z, audio and the audio row stride must be 16-byte aligned");
    if (((uintptr_t)a->window & 3) || ((uintptr_t)a->twiddle & 3) || ((uintptr_t)a->lengths & 3))
        return efts_fail(EFTS_EALIGN, "efts_istft_head: window, twiddle and lengths must be 4-byte aligned");

    HeadArgs k;
    k.z = a->z; k.lengths = a->lengths; k.window = a->window; k.twiddle = a->twiddle; k.audio = a->audio;
    k.ld_audio = a->ld_audio; k.pitch = a->pitch; k.z_rows = a->z_rows; k.len_mul = a->len_mul; k.out_len = a->out_len;
    const dim3 grid((a->out_len + EFTS_ISTFT_RUN - 1) / EFTS_ISTFT_RUN, a->B);
    if (a->n_fft == 8) hipLaunchKernelGGL(istft_head_kernel<8>, grid, dim3(256), 0, st, k);
    else if (a->n_fft == 16) hipLaunchKernelGGL(istft_head_kernel<16>, grid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL(istft_head_kernel<32>, grid, dim3(256), 0, st, k);
    return efts_check_launch("efts_istft_head");
}
