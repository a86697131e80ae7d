// efts_optim.hip -- clip_grad_norm_ + Adam / AdamW / RAdam on flat fp32 buffers, one launch (efts_optim_step).
//
// What the reference's registry resolves for `optimizer_type` (nntts/optimizers/__init__.py: all of torch.optim plus its own RAdam,
// nntts/optimizers/radam.py).  The amsgrad Adam of the shipped recipe stays in efts_train.hip (efts_adam_amsgrad, bit for bit as it was);
// this file holds every other member of the family:
//
//   ADAM   torch.optim.Adam  : gg = coef g + wd p;                 m, v;  p -= w0 m / (sqrt(vh) / w1 + eps)
//   ADAMW  torch.optim.AdamW : gg = coef g;         p *= w2;       m, v;  p -= w0 m / (sqrt(vh) / w1 + eps)
//   RADAM  radam.py          : gg = coef g;         p *= w2;       v, m;  p -= w3 ? w0 m / (sqrt(v) + eps) : w0 m
//
// with vh = amsgrad ? (vmax = max(vmax, v)) : v and the four per-step words {w0, w1, w2, w3} =
//   {lr / (1 - b1^t), sqrt(1 - b2^t), 1 or 1 - lr wd, 0}            ADAM / ADAMW
//   {lr * step_size,  1,              1 - lr wd,      rectified}     RADAM (N_sma, step_size and the branch as radam.py:66-76)
// computed on the HOST in double (optim_words: the one definition behind the by-value launch and efts_optim_hyper) -- the kernel
// carries no pow and no branch on the step number, so a captured launch that reads the words from device memory replays any step.
//
// HBM-bound: 7 words per element (p, g, m, v read; p, m, v written), 9 with amsgrad.  16-byte accesses, 256-thread blocks, at most 2048
// blocks that grid-stride (cdna_hip_programming.md Guideline 11 / 13); amsgrad and the algorithm are template parameters, so the 7-word
// variants hold no load or store of vmax.  No atomics: two runs give the same bits.
//
// Beside them, the exponential moving average of the parameters (efts_ema_update): e = fmaf(w, p - e, e) over the same flat buffer, in the
// same shape, 3 words per element (p, e read; e written), with its one per-update word w = 1 - decay from the host (efts_ema_hyper).  A
// launch of its own, not a fourth template parameter of optim_kernel: see DESIGN.md "The parameter EMA stays a launch of its own".
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "efts_internal.h"

namespace efts {

// by-value constants of one optimizer: (float) beta and (float)(1 - beta) rounded from double once, as torch's fp32 kernels receive them
struct OptimConst { float b1, omb1, b2, omb2, eps, wd; };

template <int ALGO, bool AMS>
__device__ __forceinline__ void optim_update(float& p, float g, float& m, float& v, float& vm, float coef, const OptimConst& k, const float4& w) {
    float gg = g * coef;
    if (ALGO == EFTS_OPTIM_ADAM) gg += k.wd * p;        // coupled L2
    else p *= w.z;                                      // decoupled decay
    m = k.b1 * m + k.omb1 * gg;
    v = k.b2 * v + k.omb2 * gg * gg;
    if (ALGO == EFTS_OPTIM_RADAM) {
        p -= w.w != 0.f ? w.x * m / (sqrtf(v) + k.eps) : w.x * m;
    } else {
        float vh = v;
        if (AMS) { vm = fmaxf(vm, v); vh = vm; }
        p -= w.x * m / (sqrtf(vh) / w.y + k.eps);
    }
}

// hyper (optional): the four words in device memory instead of `w` -- the step as a hipGraph
template <int ALGO, bool AMS>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, float* __restrict__ vmax, long n,
                                                    const float* __restrict__ sumsq, float max_norm, float gscale, OptimConst k, float4 w,
                                                    const float* __restrict__ hyper) {
    if (hyper) w = make_float4(hyper[0], hyper[1], hyper[2], hyper[3]);
    float coef = gscale;
    if (sumsq && max_norm > 0.f) {
        const float nrm = sqrtf(sumsq[0]) * gscale;    // norm of the (already averaged) gradient
        const float cc = max_norm / (nrm + 1e-6f);
        coef *= cc < 1.f ? cc : 1.f;
    }
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long)gridDim.x * 1024) {
        if (i + 3 < n) {
            float4 pp = *(const float4*)(p + i), mm = *(const float4*)(m + i), vv = *(const float4*)(v + i);
            const float4 gg = *(const float4*)(g + i);
            float4 vm = AMS ? *(const float4*)(vmax + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            optim_update<ALGO, AMS>(pp.x, gg.x, mm.x, vv.x, vm.x, coef, k, w);
            optim_update<ALGO, AMS>(pp.y, gg.y, mm.y, vv.y, vm.y, coef, k, w);
            optim_update<ALGO, AMS>(pp.z, gg.z, mm.z, vv.z, vm.z, coef, k, w);
            optim_update<ALGO, AMS>(pp.w, gg.w, mm.w, vv.w, vm.w, coef, k, w);
            *(float4*)(p + i) = pp; *(float4*)(m + i) = mm; *(float4*)(v + i) = vv;
            if (AMS) *(float4*)(vmax + i) = vm;
        } else {
            for (long j = i; j < n; ++j) {
                float pp = p[j], mm = m[j], vv = v[j], vm = AMS ? vmax[j] : 0.f;
                optim_update<ALGO, AMS>(pp, g[j], mm, vv, vm, coef, k, w);
                p[j] = pp; m[j] = mm; v[j] = vv;
                if (AMS) vmax[j] = vm;
            }
        }
    }
}

// e += w (p - e): d = fl(p - e), one fp32 subtraction, then e' = fl(w d + e), one fma.  The two ends mean what they say rather than what
// the formula rounds to: w == 0 writes nothing, w == 1 stores p (fl(fl(p - e) + e) is not p where |p| is far below |e|).
__device__ __forceinline__ float ema_apply(float e, float p, float w) { return w == 1.f ? p : fmaf(w, p - e, e); }

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ e, const float* __restrict__ p, long n, float w) {
    if (w == 0.f) return;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long)gridDim.x * 1024) {
        if (i + 3 < n) {
            const float4 pp = *(const float4*)(p + i);
            float4 ee = *(const float4*)(e + i);
            ee.x = ema_apply(ee.x, pp.x, w);
            ee.y = ema_apply(ee.y, pp.y, w);
            ee.z = ema_apply(ee.z, pp.z, w);
            ee.w = ema_apply(ee.w, pp.w, w);
            *(float4*)(e + i) = ee;
        } else {
            for (long j = i; j < n; ++j) e[j] = ema_apply(e[j], p[j], w);
        }
    }
}

}  // namespace efts

using namespace efts;
#define ST ((hipStream_t)stream)

// the four per-step words, in double as torch's / radam.py's Python floats, rounded to fp32 once
static void optim_words(int algo, double lr, double b1, double b2, double wd, int step, float* w) {
    const double bc1 = 1.0 - pow(b1, (double)step), b2t = pow(b2, (double)step);
    if (algo == EFTS_OPTIM_RADAM) {
        const double nmax = 2.0 / (1.0 - b2) - 1.0;
        const double nsma = nmax - 2.0 * step * b2t / (1.0 - b2t);
        const bool rect = nsma >= 5.0;
        const double ss = rect ? sqrt((1.0 - b2t) * (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma * nmax / (nmax - 2.0)) / bc1 : 1.0 / bc1;
        w[0] = (float)(ss * lr); w[1] = 1.f; w[2] = (float)(1.0 - wd * lr); w[3] = rect ? 1.f : 0.f;
    } else {
        w[0] = (float)(lr / bc1); w[1] = (float)sqrt(1.0 - b2t); w[2] = algo == EFTS_OPTIM_ADAMW ? (float)(1.0 - lr * wd) : 1.f; w[3] = 0.f;
    }
}

static bool optim_hyper_ok(int algo, double b1, double b2) {
    return algo >= EFTS_OPTIM_ADAM && algo <= EFTS_OPTIM_RADAM && b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0;
}

extern "C" int efts_optim_hyper(int32_t algo, double lr, double beta1, double beta2, double weight_decay, int32_t step, float* out4) {
    if (!out4 || step < 1 || !optim_hyper_ok(algo, beta1, beta2))
        return efts_fail(EFTS_EINVAL, "efts_optim_hyper: out4 NULL, step < 1, unknown algo or a beta outside [0, 1)");
    optim_words(algo, lr, beta1, beta2, weight_decay, step, out4);
    return EFTS_OK;
}

template <int ALGO, bool AMS>
static void optim_launch(const efts_optim_args* a, const OptimConst& k, float4 w, void* stream) {
    const long blocks = (a->n + 1023) / 1024;
    hipLaunchKernelGGL((optim_kernel<ALGO, AMS>), dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, ST, a->p, a->g, a->m, a->v,
                       AMS ? a->vmax : (float*)nullptr, (long)a->n, a->sumsq, a->max_norm, a->gscale, k, w, a->hyper);
}

extern "C" int efts_optim_step(const efts_optim_args* a, void* stream) {
    if (!a) return efts_fail(EFTS_EINVAL, "efts_optim_step: null argument block");
    if (!a->p || !a->g || !a->m || !a->v || a->n <= 0) return efts_fail(EFTS_EINVAL, "efts_optim_step: null pointer or n <= 0");
    if (!optim_hyper_ok(a->algo, a->beta1, a->beta2)) return efts_fail(EFTS_EINVAL, "efts_optim_step: unknown algo (%d) or a beta outside [0, 1)", a->algo);
    if (a->amsgrad && a->algo == EFTS_OPTIM_RADAM) return efts_fail(EFTS_EINVAL, "efts_optim_step: RADAM has no amsgrad form");
    if (a->amsgrad && !a->vmax) return efts_fail(EFTS_EINVAL, "efts_optim_step: amsgrad needs vmax");
    if (!a->hyper && a->step < 1) return efts_fail(EFTS_EINVAL, "efts_optim_step: step must be >= 1 (got %d)", a->step);
    if (((uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m | (uintptr_t)a->v | (a->amsgrad ? (uintptr_t)a->vmax : 0)) & 15)
        return efts_fail(EFTS_EALIGN, "efts_optim_step: buffers must be 16-byte aligned");
    if ((uintptr_t)a->hyper & 3 || (uintptr_t)a->sumsq & 3) return efts_fail(EFTS_EALIGN, "efts_optim_step: hyper / sumsq must be 4-byte aligned");
    const OptimConst k = {(float)a->beta1, (float)(1.0 - a->beta1), (float)a->beta2, (float)(1.0 - a->beta2), (float)a->eps, (float)a->weight_decay};
    float w[4] = {0.f, 1.f, 1.f, 0.f};
    if (!a->hyper) optim_words(a->algo, a->lr, a->beta1, a->beta2, a->weight_decay, a->step, w);
    const float4 w4 = make_float4(w[0], w[1], w[2], w[3]);
    switch (a->algo * 2 + (a->amsgrad ? 1 : 0)) {
        case EFTS_OPTIM_ADAM * 2: optim_launch<EFTS_OPTIM_ADAM, false>(a, k, w4, stream); break;
        case EFTS_OPTIM_ADAM * 2 + 1: optim_launch<EFTS_OPTIM_ADAM, true>(a, k, w4, stream); break;
        case EFTS_OPTIM_ADAMW * 2: optim_launch<EFTS_OPTIM_ADAMW, false>(a, k, w4, stream); break;
        case EFTS_OPTIM_ADAMW * 2 + 1: optim_launch<EFTS_OPTIM_ADAMW, true>(a, k, w4, stream); break;
        default: optim_launch<EFTS_OPTIM_RADAM, false>(a, k, w4, stream); break;
    }
    return efts_check_launch("efts_optim_step");
}

// the per-update word of the parameter EMA, in double as Python floats, rounded to fp32 once
extern "C" int efts_ema_hyper(double decay, int32_t warmup, int64_t updates, float* out1) {
    if (!out1 || !(decay >= 0.0 && decay < 1.0) || updates < 0)
        return efts_fail(EFTS_EINVAL, "efts_ema_hyper: out1 NULL, decay outside [0, 1) or updates < 0");
    double d = decay;
    if (warmup) {
        const double ramp = (1.0 + (double)updates) / (10.0 + (double)updates);
        if (ramp < d) d = ramp;
    }
    out1[0] = (float)(1.0 - d);
    return EFTS_OK;
}

extern "C" int efts_ema_update(float* ema, const float* p, int64_t n, float one_minus_decay, void* stream) {
    if (!ema || !p || n <= 0) return efts_fail(EFTS_EINVAL, "efts_ema_update: null pointer or n <= 0");
    if (!(one_minus_decay >= 0.f && one_minus_decay <= 1.f))
        return efts_fail(EFTS_EINVAL, "efts_ema_update: one_minus_decay must lie in [0, 1] (got %g)", (double)one_minus_decay);
    if (((uintptr_t)ema | (uintptr_t)p) & 15) return efts_fail(EFTS_EALIGN, "efts_ema_update: buffers must be 16-byte aligned");
    const long blocks = ((long)n + 1023) / 1024;
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, ST, ema, p, (long)n, one_minus_decay);
    return efts_check_launch("efts_ema_update");
}
