// Training step: gradient accumulation over micro-batches (Lightning's `accumulate_grad_batches`), acc += weight * g over the flat
// gradient buffer.  The operators' backward OVERWRITES the flat gradient buffer (one backward per zeroed buffer), so the running sum
// lives in a buffer of its own and this is the one kernel that adds to it; no weight-gradient or reduction kernel has an accumulate
// mode.  tu_train.hip includes this header itself, behind train_ops.h.
#pragma once
#include "esmi_dev.h"

namespace esmi {

// acc[q] = fmaf(g[q], w, acc[q]) for q < n: one rounding per element, every element owned by exactly one lane, no atomics -- the same
// inputs give the same bits.  At most 1024 workgroups of 256 stride over n4 whole float4s (16 bytes per lane; the launcher passes
// n4 = 0 unless BOTH pointers are 16-byte aligned) and then over the scalar tail [4 n4, n).  Nothing at or beyond n is read or
// written.  inf and nan in g arrive in acc (the precision-16 skip rule reads them there).
static __global__ __launch_bounds__(256) void train_grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n4,
                                                                           long n, float w) {
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    for (long q = tid; q < n4; q += nth) {
        const f32x4 x = ld4(g + q * 4);
        f32x4 a = ld4(acc + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = fmaf(x[e], w, a[e]);
        *reinterpret_cast<f32x4*>(acc + q * 4) = a;
    }
    for (long q = n4 * 4 + tid; q < n; q += nth) acc[q] = fmaf(g[q], w, acc[q]);
}

}  // namespace esmi
