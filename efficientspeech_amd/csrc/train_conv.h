// Training step: the convolution descriptor, the scalar forward / data-gradient kernels, the depthwise kernel and the batched
// weight pack.  Activations are channels-last (B, n, C); weights stay in CHECKPOINT layout (what the optimizer updates):
// Conv1d (Cout, Cin/groups, k), ConvTranspose1d (Cin, Cout, k), Linear (Cout, Cin) = Conv1d with k = 1.  Dense shapes run on the
// matrix pipe instead (convgemm.h, through tu_train.hip conv_gemm); the two one-thread-per-output kernels here take the rest.
#pragma once
#include "esmi_dev.h"

namespace esmi {

struct ConvDesc {   // mirrors esmi_conv_desc (include/esmi.h), without its trailing `precision` (a property of the GEMM launch)
    int B, n_in, c_in, n_out, c_out, k, stride, pad, groups, transposed;
};

// weight element for (output channel co, input channel ci, tap j); false when the pair is not connected (grouped conv)
__device__ __forceinline__ bool conv_w_index(const ConvDesc& d, int co, int ci, int j, long* idx) {
    if (d.transposed) { *idx = ((long)ci * d.c_out + co) * d.k + j; return true; }        // (Cin, Cout, k), groups == 1
    const int cig = d.c_in / d.groups, cog = d.c_out / d.groups;
    const int g = co / cog;
    if (ci / cig != g) return false;
    *idx = ((long)co * cig + (ci - g * cig)) * d.k + j;                                     // (Cout, Cin/groups, k)
    return true;
}
// input position feeding output position t through tap j (or -1)
__device__ __forceinline__ int conv_in_pos(const ConvDesc& d, int t, int j) {
    if (!d.transposed) {
        const int ti = t * d.stride + j - d.pad;
        return (ti >= 0 && ti < d.n_in) ? ti : -1;
    }
    const int q = t + d.pad - j;                      // ConvTranspose1d: out[n*stride + j - pad] += in[n] * W[:, :, j]
    if (q < 0 || q % d.stride) return -1;
    const int ti = q / d.stride;
    return ti < d.n_in ? ti : -1;
}

// y[b, t, co] = bias[co] + sum_j sum_ci x[b, in_pos(t, j), ci] * w(co, ci, j)
static __global__ void train_conv_fwd_kernel(const ConvDesc d, const float* __restrict__ x, const float* __restrict__ w,
                                      const float* __restrict__ bias, float* __restrict__ y) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)d.B * d.n_out * d.c_out) return;
    const int co = (int)(q % d.c_out), t = (int)((q / d.c_out) % d.n_out), b = (int)(q / ((long)d.c_out * d.n_out));
    const int cig = d.transposed ? d.c_in : d.c_in / d.groups, ci0 = d.transposed ? 0 : (co / (d.c_out / d.groups)) * cig;
    float acc = bias ? bias[co] : 0.0f;
    for (int j = 0; j < d.k; ++j) {
        const int ti = conv_in_pos(d, t, j);
        if (ti < 0) continue;
        const float* xr = x + ((long)b * d.n_in + ti) * d.c_in;
        for (int c = 0; c < cig; ++c) {
            long wi;
            conv_w_index(d, co, ci0 + c, j, &wi);
            acc = fmaf(xr[ci0 + c], w[wi], acc);
        }
    }
    y[q] = acc;
}

// depthwise, stride 1 (MelDecoder's k = 5 convs): one thread per (kDwRows consecutive rows, 4 channels), 16-byte accesses -- the rows
// slide through registers (kDwRows + k - 1 loads for kDwRows outputs instead of k each), the k x 4 weights are read once.  `grad`
// runs the data gradient: dx[t] = sum_j dy[t + pad - j] w[j] = the same correlation with the taps reversed and padding k - 1 - pad.
// Requires k <= 8; weights (C, 1, k)
constexpr int kDwRows = 8;
static __global__ __launch_bounds__(256) void train_conv_dw_kernel(const ConvDesc d, const float* __restrict__ in, const float* __restrict__ w,
                                     const float* __restrict__ bias, float* __restrict__ out, int grad) {
    const int c4 = d.c_out >> 2;
    const int n_o = grad ? d.n_in : d.n_out, n_i = grad ? d.n_out : d.n_in;
    const int tb = (n_o + kDwRows - 1) / kDwRows;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)d.B * tb * c4) return;
    const int c = (int)(q % c4) * 4, t0 = (int)((q / c4) % tb) * kDwRows, b = (int)(q / ((long)c4 * tb));
    const int pad = grad ? d.k - 1 - d.pad : d.pad;
    f32x4 wt[8];                                       // wt[j][e]: tap j of channel c + e, in correlation order
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) wt[j][e] = j < d.k ? w[(long)(c + e) * d.k + (grad ? d.k - 1 - j : j)] : 0.0f;
    }
    const f32x4 b4 = (bias && !grad) ? ld4(bias + c) : zero4();
    f32x4 acc[kDwRows];
#pragma unroll
    for (int o = 0; o < kDwRows; ++o) acc[o] = b4;
    const float* base = in + (long)b * n_i * d.c_out + c;
    // every input row first, unconditionally (clamped into the utterance, zeroed where outside: round 5 -- a load under a per-row
    // condition is waited for before the next one is issued), then the products: row t0 - pad + r feeds output o through tap j = r - o
    f32x4 v[kDwRows + 7];
#pragma unroll
    for (int r = 0; r < kDwRows + 7; ++r) {
        const int ti = t0 - pad + r, tc = ti < 0 ? 0 : (ti >= n_i ? n_i - 1 : ti);
        v[r] = r < kDwRows + d.k - 1 ? ld4(base + (long)tc * d.c_out) : zero4();
        if (ti != tc) v[r] = zero4();
    }
#pragma unroll
    for (int r = 0; r < kDwRows + 7; ++r) {
#pragma unroll
        for (int o = 0; o < kDwRows; ++o) {
            const int j = r - o;
            if (j >= 0 && j < 8) {                     // (compile-time after unrolling; taps >= k hold zero weights)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[o][e] = fmaf(v[r][e], wt[j][e], acc[o][e]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < kDwRows; ++o)
        if (t0 + o < n_o) *reinterpret_cast<f32x4*>(out + ((long)b * n_o + t0 + o) * d.c_out + c) = acc[o];
}

// dx[b, ti, ci] = sum over (t, j) with in_pos(t, j) == ti, and co connected to ci, of dy[b, t, co] * w(co, ci, j)
static __global__ void train_conv_dgrad_kernel(const ConvDesc d, const float* __restrict__ dy, const float* __restrict__ w,
                                        float* __restrict__ dx) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)d.B * d.n_in * d.c_in) return;
    const int ci = (int)(q % d.c_in), ti = (int)((q / d.c_in) % d.n_in), b = (int)(q / ((long)d.c_in * d.n_in));
    const int cog = d.transposed ? d.c_out : d.c_out / d.groups, co0 = d.transposed ? 0 : (ci / (d.c_in / d.groups)) * cog;
    float acc = 0.0f;
    for (int j = 0; j < d.k; ++j) {
        int t;
        if (!d.transposed) {                          // ti = t*stride + j - pad
            const int r = ti + d.pad - j;
            if (r < 0 || r % d.stride) continue;
            t = r / d.stride;
        } else {                                      // t = ti*stride + j - pad
            t = ti * d.stride + j - d.pad;
        }
        if (t < 0 || t >= d.n_out) continue;
        const float* dr = dy + ((long)b * d.n_out + t) * d.c_out;
        for (int c = 0; c < cog; ++c) {
            long wi;
            conv_w_index(d, co0 + c, ci, j, &wi);
            acc = fmaf(dr[co0 + c], w[wi], acc);
        }
    }
    dx[q] = acc;
}

// tap-major GEMM copies of many weights in one launch (blockIdx.y = item): what pack_conv_kernel does per convolution
struct PackItem { const float* src; float* dst; int* zero_slot; int cout, cin, k, transposed, flip; };
constexpr int kPackBatch = 64;
struct PackBatch { int count; PackItem items[kPackBatch]; };
static __global__ void train_pack_batch_kernel(const PackBatch b) {
    const PackItem& it = b.items[blockIdx.y];
    if (it.zero_slot && blockIdx.x == 0 && threadIdx.x == 0) it.zero_slot[0] = 0;
    const long n = (long)it.cout * it.cin * it.k;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e % it.cin);
        const int o = (int)((e / it.cin) % it.cout);
        const int j = (int)(e / ((long)it.cin * it.cout));
        const int js = it.flip ? it.k - 1 - j : j;
        it.dst[e] = it.transposed ? it.src[((long)i * it.cout + o) * it.k + js] : it.src[((long)o * it.cin + i) * it.k + js];
    }
}

}  // namespace esmi
