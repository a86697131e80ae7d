// efts_stft_frame.h -- the framing that the STFT kernels share (efts_stft.hip, efts_mcep.hip): centred frames, reflect padding without edge
// repeat, the int16 scaling and the window at the loads, two neighbouring frames as the real and imaginary part of one transform.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "efts_fft.h"

namespace efts {

// index i of the centred, reflect-padded signal (reflection without edge repeat; len > N / 2 keeps one reflection enough)
__device__ __forceinline__ int st_reflect(int s, int len) {
    s = s < 0 ? -s : s;
    s = s >= len ? 2 * (len - 1) - s : s;
    return min(max(s, 0), len - 1);            // (out of range only for a frame past the item's count, whose values are dropped)
}

// v[n1] = (frame a, frame b)[G n1 + l] times the window; frame a begins at sample s0 of the un-padded signal, frame b one hop later
template <typename S, int N, int M, int G>
__device__ __forceinline__ void st_load(const S* __restrict__ a, float scale, int len, int s0, int H, bool vb, int l, const float (&win)[M], fft::cf (&v)[M]) {
    if (s0 >= 0 && s0 + H + N <= len) {        // (uniform in the group) both frames lie inside the item: one base, constant offsets
        const S* p = a + s0 + l;
#pragma unroll
        for (int n1 = 0; n1 < M; ++n1) v[n1] = fft::cf{(float)p[G * n1] * scale * win[n1], (float)p[G * n1 + H] * scale * win[n1]};
    } else {
#pragma unroll
        for (int n1 = 0; n1 < M; ++n1) {
            const int i = s0 + G * n1 + l;
            const float xa = (float)a[st_reflect(i, len)] * scale, xb = (float)a[st_reflect(i + H, len)] * scale;
            v[n1] = fft::cf{xa * win[n1], vb ? xb * win[n1] : 0.f};
        }
    }
}

}  // namespace efts
