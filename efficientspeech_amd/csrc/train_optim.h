// Training step: AdamW, torch.optim.AdamW's arithmetic (decoupled decay first, bias corrections as two scalars), over a flat buffer;
// the one-thread bookkeeping of the device-scalar variants (step counter, GradScaler state, clipping) and the gradient norm.
// Every scalar is derived in double precision (host, or one device thread for the graph variant) and rounded to fp32 once.
#pragma once
#include "train_reduce.h"

namespace esmi {

struct AdamWScalars { float beta1, one_m_beta1, beta2, one_m_beta2, eps, decay /* 1 - lr wd */, step_size /* lr / bc1 */, bc2_sqrt, gscale; };

__device__ __forceinline__ void adamw_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, long q, const AdamWScalars& h) {
    const float grad = g[q] * h.gscale;
    float w = p[q] * h.decay;
    const float mm = h.beta1 * m[q] + h.one_m_beta1 * grad;
    const float vv = h.beta2 * v[q] + h.one_m_beta2 * grad * grad;
    m[q] = mm;
    v[q] = vv;
    const float denom = sqrtf(vv) / h.bc2_sqrt + h.eps;
    w -= h.step_size * (mm / denom);
    p[q] = w;
}

static __global__ void train_adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                   long n, AdamWScalars h) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) adamw_update(p, g, m, v, q, h);
}

// the same with the step count and the learning rate read from device memory, so that a captured hipGraph of the whole
// training step replays correctly -- and so that `precision=16`'s dynamic loss scaling needs no host round trip:
//   hyper  = {lr (caller), 1 - lr wd, lr / bc1, sqrt(bc2), skip flag, gradient scale, gradient norm, clip coefficient}  (all but the first
//            written by train_bump_step_kernel, the last two by its clipping twin only; the slots' names: ESMI_HYPER_* and ESMI_SCALER_*
//            in include/esmi.h)
//   scaler = NULL, or torch.amp.GradScaler's state {scale, growth_factor, backoff_factor, growth_interval, clean steps in a row,
//            skipped steps}: an inf / nan in the (scaled) gradients -- `grad_absmax` holds max|g| with nan ordered as inf -- skips the
//            update (the step counter does not advance), multiplies the scale by backoff_factor; growth_interval clean steps in a
//            row multiply it by growth_factor (GradScaler.step + .update, torch/amp/grad_scaler.py)
//   clip   = false, or torch.nn.utils.clip_grad_norm_(params, max_norm, 2) between GradScaler's unscale_ and the update (Lightning's
//            `gradient_clip_val`): `sumsq` = sum g^2 over the (still scaled) gradient buffer, so total = sqrt(sumsq) / scale is the norm of
//            the unscaled gradients; coef = min(1, max_norm / (total + 1e-6)) in fp32 as torch forms it, and the update runs on
//            g * (coef / scale).  total and coef are left in hyper[ESMI_HYPER_GRAD_NORM] / [ESMI_HYPER_CLIP_COEF].  The skip rule above is
//            untouched (a skipped step records whatever non-finite norm came out); WITHOUT a scaler a non-finite norm makes coef nan and
//            poisons the update, as in torch -- no skip is invented here.
// (one thread: every store below is an ordinary per-lane global store)
__device__ __forceinline__ void bump_step(int* __restrict__ step, float* __restrict__ hyper, double beta1, double beta2, double wd,
                                          const float* __restrict__ grad_absmax, float* __restrict__ scaler, bool clip, double sumsq,
                                          double max_norm) {
    bool skip = false;
    float gscale = 1.0f;
    if (clip) {
        const float scale = scaler ? scaler[ESMI_SCALER_SCALE] : 1.0f;
        const float total = (float)(sqrt(sumsq) / (double)scale);
        const float c = (float)max_norm / (total + 1e-6f);
        const float coef = c > 1.0f ? 1.0f : c;         // (torch.clamp(max=1.0): nan stays nan)
        hyper[ESMI_HYPER_GRAD_NORM] = total;
        hyper[ESMI_HYPER_CLIP_COEF] = coef;
        gscale = coef;
    }
    if (scaler) {
        const float amax = grad_absmax[0], scale = scaler[ESMI_SCALER_SCALE];
        if (!(amax <= 3.4028234663852886e38f)) {       // inf or nan
            gscale = 1.0f;
            skip = true;
            scaler[ESMI_SCALER_SCALE] = scale * scaler[ESMI_SCALER_BACKOFF_FACTOR];
            scaler[ESMI_SCALER_CLEAN_STEPS] = 0.0f;
            scaler[ESMI_SCALER_SKIPPED] += 1.0f;
        } else {
            gscale = gscale / scale;                   // (1 / scale without clipping; coef / scale, rounded once, with it)
            float good = scaler[ESMI_SCALER_CLEAN_STEPS] + 1.0f;
            if (good >= scaler[ESMI_SCALER_GROWTH_INTERVAL]) {
                scaler[ESMI_SCALER_SCALE] = scale * scaler[ESMI_SCALER_GROWTH_FACTOR];
                good = 0.0f;
            }
            scaler[ESMI_SCALER_CLEAN_STEPS] = good;
        }
    }
    hyper[ESMI_HYPER_SKIP] = skip ? 1.0f : 0.0f;
    hyper[ESMI_HYPER_GRAD_SCALE] = gscale;
    if (skip) return;
    const int t = step[0] + 1;
    step[0] = t;
    const double lr = (double)hyper[ESMI_HYPER_LR];
    const double bc1 = -expm1((double)t * log(beta1)), bc2 = -expm1((double)t * log(beta2));
    hyper[ESMI_HYPER_DECAY] = (float)(1.0 - lr * wd);
    hyper[ESMI_HYPER_STEP_SIZE] = (float)(lr / bc1);
    hyper[ESMI_HYPER_BC2_SQRT] = (float)sqrt(bc2);
}
static __global__ void train_bump_step_kernel(int* __restrict__ step, float* __restrict__ hyper, double beta1, double beta2, double wd,
                                              const float* __restrict__ grad_absmax, float* __restrict__ scaler) {
    if (threadIdx.x != 0) return;
    bump_step(step, hyper, beta1, beta2, wd, grad_absmax, scaler, false, 0.0, 0.0);
}

// ---- the gradient norm for clipping, in two deterministic stages (no atomics: the same buffer gives the same bits on every run).
// Stage 1: at most ESMI_TRAIN_GRAD_NORM_PARTIALS workgroups of 256 stride over the flat fp32 buffer 16 bytes per lane at a time (n4
// whole float4s; 0 when the buffer is not 16-byte aligned) and then over the scalar tail [4 n4, n).  Every square is formed and added
// in double: the product of two fp32 values is exact there, so neither a gradient of 1e-30 nor one of 1e30 leaves the sum.  Each
// workgroup stores one partial; workgroup 0 also zeroes the slots behind the grid, so that stage 2 always adds all of them.
static __global__ __launch_bounds__(256) void train_grad_sumsq_kernel(const float* __restrict__ g, long n4, long n,
                                                                      double* __restrict__ partials) {
    ESMI_DYN_LDS(red_f);   // 256 doubles
    double* red = reinterpret_cast<double*>(red_f);
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    double acc = 0.0;
    for (long q = tid; q < n4; q += nth) {
        const f32x4 x = ld4(g + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fma((double)x[e], (double)x[e], acc);
    }
    for (long q = n4 * 4 + tid; q < n; q += nth) acc = fma((double)g[q], (double)g[q], acc);
    const double t = block_sum_256(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    if (blockIdx.x == 0)
        for (int j = (int)gridDim.x + (int)threadIdx.x; j < ESMI_TRAIN_GRAD_NORM_PARTIALS; j += 256) partials[j] = 0.0;
}
// Stage 2 rides in the optimizer's one-workgroup bookkeeping launch: 256 threads add the partials in a fixed order (four each, then
// the tree), thread 0 then does what train_bump_step_kernel does, with the clip coefficient folded into the gradient scale.
static __global__ __launch_bounds__(256) void train_bump_clip_kernel(int* __restrict__ step, float* __restrict__ hyper, double beta1,
                                                                     double beta2, double wd, const float* __restrict__ grad_absmax,
                                                                     float* __restrict__ scaler, const double* __restrict__ partials,
                                                                     double max_norm) {
    ESMI_DYN_LDS(red_f);   // 256 doubles
    double acc = 0.0;
    for (int j = (int)threadIdx.x; j < ESMI_TRAIN_GRAD_NORM_PARTIALS; j += 256) acc += partials[j];
    const double sumsq = block_sum_256(acc, reinterpret_cast<double*>(red_f));
    if (threadIdx.x != 0) return;
    bump_step(step, hyper, beta1, beta2, wd, grad_absmax, scaler, true, sumsq, max_norm);
}
static __global__ void train_adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                       long n, AdamWScalars h, const float* __restrict__ hyper) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n || hyper[ESMI_HYPER_SKIP] != 0.0f) return;
    h.decay = hyper[ESMI_HYPER_DECAY];
    h.step_size = hyper[ESMI_HYPER_STEP_SIZE];
    h.bc2_sqrt = hyper[ESMI_HYPER_BC2_SQRT];
    h.gscale = hyper[ESMI_HYPER_GRAD_SCALE];
    adamw_update(p, g, m, v, q, h);
}

}  // namespace esmi
