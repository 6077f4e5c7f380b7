// Training step: an exponential moving average of the weights (torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(decay),
// Lightning's weight averaging) over the flat parameter buffer, and the in-place exchange that lets the model run on it.  The
// parameters are views of the flat buffer, and packed copies and captured graphs hold its address, so "load the average" exchanges
// CONTENTS; no pointer moves.  tu_train.hip includes this header itself, behind train_ops.h, as it does train_accum.h.
#pragma once
#include "esmi_dev.h"

namespace esmi {

// ema[q] = fmaf(w, p[q] - ema[q], ema[q]) for q < n, w = 1 - decay: torch.lerp(ema, p, w)'s form for w < 0.5, one subtraction and one
// fused multiply-add.  Geometry as train_grad_accumulate_kernel's: at most 1024 workgroups of 256 stride over n4 whole float4s (the
// launcher passes n4 = 0 unless BOTH pointers are 16-byte aligned) and then over the scalar tail [4 n4, n); every element has one
// owner, no atomics, no LDS; nothing at or beyond n is read or written.  hyper != NULL: the optimizer launch's hyper block -- every
// lane reads its skip flag first (one uniform load) and a skipped precision-16 step leaves the average alone, as it leaves the step
// counter alone.  inf and nan in p arrive in ema.
static __global__ __launch_bounds__(256) void train_ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n4, long n,
                                                                      float w, const float* __restrict__ hyper) {
    if (hyper != nullptr && hyper[ESMI_HYPER_SKIP] != 0.0f) return;
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    for (long q = tid; q < n4; q += nth) {
        const f32x4 x = ld4(p + q * 4);
        f32x4 a = ld4(ema + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = fmaf(w, x[e] - a[e], a[e]);
        *reinterpret_cast<f32x4*>(ema + q * 4) = a;
    }
    for (long q = n4 * 4 + tid; q < n; q += nth) ema[q] = fmaf(w, p[q] - ema[q], ema[q]);
}

// a[q] <-> b[q] for q < n in one launch, no temporary buffer: each lane holds its own elements of both in registers between the loads
// and the stores.  The same geometry and alignment rule.  Loads and stores only, so every bit travels (nan payloads, -0.0): two swaps
// restore both buffers exactly.
static __global__ __launch_bounds__(256) void train_swap_kernel(float* __restrict__ a, float* __restrict__ b, long n4, long n) {
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    for (long q = tid; q < n4; q += nth) {
        const f32x4 x = ld4(a + q * 4), y = ld4(b + q * 4);
        *reinterpret_cast<f32x4*>(a + q * 4) = y;
        *reinterpret_cast<f32x4*>(b + q * 4) = x;
    }
    for (long q = n4 * 4 + tid; q < n; q += nth) {
        const float x = a[q], y = b[q];
        a[q] = y;
        b[q] = x;
    }
}

}  // namespace esmi
