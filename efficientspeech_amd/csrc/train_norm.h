// Training step: LayerNorm over the last dim (biased variance, eps inside the sqrt), forward and backward, and the stand-alone
// activations.  One wave per row with the lanes across the channels (coalesced), or LPR lanes per row with the row in registers;
// the row sums by a fixed butterfly (train_reduce.h); mean / rstd kept for backward.
#pragma once
#include "train_reduce.h"

namespace esmi {

// res != NULL: the normalised tensor is x + res, written to `xsum` for the backward (LN(f(x) + x), networks.py:75,83,301);
// rowmask[r] != 0: the output row is zero (masked_fill after the norm, networks.py:76,84) -- the backward kernels take the same mask
// (x and y are NOT __restrict__: the two-launch conv + LayerNorm fallback of train.py runs the norm in place, x == y; every lane reads
// its elements of a row before it writes them)
static __global__ __launch_bounds__(256) void train_ln_fwd_kernel(const float* x, const float* __restrict__ g,
                                                           const float* __restrict__ b, long rows, int C, float eps,
                                                           float* y, float* __restrict__ mean, float* __restrict__ rstd,
                                                           const float* __restrict__ res, float* __restrict__ xsum,
                                                           const unsigned char* __restrict__ rowmask, int relu_out) {
    const long r = (long)blockIdx.x * 4 + wave_id();
    if (r >= rows) return;
    const int lane = lane_id();
    const float* xr = x + r * C;
    float m = 0.0f;
    if (res) {   // this lane re-reads only what it wrote
        for (int c = lane; c < C; c += 64) { const float v = xr[c] + res[r * C + c]; xsum[r * C + c] = v; m += v; }
        xr = xsum + r * C;
    } else {
        for (int c = lane; c < C; c += 64) m += xr[c];
    }
    m = wave_sum(m) / (float)C;
    float v = 0.0f;
    for (int c = lane; c < C; c += 64) { const float dlt = xr[c] - m; v = fmaf(dlt, dlt, v); }
    const float rs = 1.0f / sqrtf(wave_sum(v) / (float)C + eps);
    if (lane == 0) { mean[r] = m; rstd[r] = rs; }
    const bool masked = rowmask && rowmask[r];
    for (int c = lane; c < C; c += 64) {
        const float v = fmaf((xr[c] - m) * rs, g[c], b[c]);
        y[r * C + c] = masked ? 0.0f : (relu_out ? fmaxf(v, 0.0f) : v);
    }
}
// The same for C = 4 LPR in {32, 64, 128, 256} on 16-byte aligned tensors: LPR lanes per row hold the row in registers (one read of
// x instead of three, 16-byte accesses), 64 / LPR rows per wave.  (The scalar form moves 78 MB in 30 us at B = 128.)
template <int LPR>
static __global__ __launch_bounds__(256) void train_ln_fwd4_kernel(const float* x, const float* __restrict__ g,
                                                            const float* __restrict__ b, long rows, float eps,
                                                            float* y, float* __restrict__ mean, float* __restrict__ rstd,
                                                            const float* __restrict__ res, float* __restrict__ xsum,
                                                            const unsigned char* __restrict__ rowmask, int relu_out) {
    constexpr int RPW = 64 / LPR, C = 4 * LPR;
    const int lane = lane_id(), sub = lane / LPR, l = lane % LPR;
    const long r = ((long)blockIdx.x * 4 + wave_id()) * RPW + sub;
    const bool live = r < rows;                        // (no early exit: the row sums are wave collectives)
    const long rc = live ? r : rows - 1;
    f32x4 v = ld4(x + rc * C + 4 * l);
    if (res) {
        v = v + ld4(res + rc * C + 4 * l);
        if (live) *reinterpret_cast<f32x4*>(xsum + rc * C + 4 * l) = v;
    }
    const float m = group_sum<LPR>((v[0] + v[1]) + (v[2] + v[3])) / (float)C;
    f32x4 dl;
#pragma unroll
    for (int e = 0; e < 4; ++e) dl[e] = v[e] - m;
    const float q = group_sum<LPR>(fmaf(dl[3], dl[3], fmaf(dl[2], dl[2], fmaf(dl[1], dl[1], dl[0] * dl[0]))));
    const float rs = 1.0f / sqrtf(q / (float)C + eps);
    if (l == 0 && live) { mean[r] = m; rstd[r] = rs; }
    const bool masked = rowmask && rowmask[rc];
    const f32x4 gv = ld4(g + 4 * l), bv = ld4(b + 4 * l);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = fmaf(dl[e] * rs, gv[e], bv[e]);
        o[e] = masked ? 0.0f : (relu_out ? fmaxf(t, 0.0f) : t);
    }
    if (live) *reinterpret_cast<f32x4*>(y + rc * C + 4 * l) = o;
}
// derivative of ReLU / tanh from the activation's OUTPUT y (kind as esmi_dev.h Act; 0: 1)
__device__ __forceinline__ float act_grad_from_output(int kind, float y) {
    return kind == ACT_RELU ? (y > 0.0f ? 1.0f : 0.0f) : (kind == ACT_TANH ? 1.0f - y * y : 1.0f);
}
// The gate on dy under relu(LN(.)) (y_relu != NULL: that output), the same in the four backward kernels: dy counts only where the
// forward's output is positive.  (Only this predicate is shared.  Each kernel folds the row mask in its own way -- an early exit, one
// bit per loaded row, one condition with the channel bound -- and one function for both moved the register counts of the fused and
// the parameter kernel: profiles/r21_train_ops_split.md.)
__device__ __forceinline__ bool relu_passes(float y) { return y > 0.0f; }
// in_act: x is the output of that activation (LN(tanh(conv)), networks.py:298; LN(relu(conv)), :152-153) and dx is returned for the
// PRE-activation tensor -- the activation's backward rides in this launch
static __global__ __launch_bounds__(256) void train_ln_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ dy, long rows, int C, float* __restrict__ dx,
                                                              const unsigned char* __restrict__ rowmask, int in_act,
                                                              const float* __restrict__ y_relu) {
    const long r = (long)blockIdx.x * 4 + wave_id();
    if (r >= rows) return;
    const int lane = lane_id();
    if (rowmask && rowmask[r]) {   // the forward zeroed this row: no gradient passes
        for (int c = lane; c < C; c += 64) dx[r * C + c] = 0.0f;
        return;
    }
    const float m = mean[r], rs = rstd[r];
    float s1 = 0.0f, s2 = 0.0f;
    for (int c = lane; c < C; c += 64) {
        const float dyv = (y_relu && !relu_passes(y_relu[r * C + c])) ? 0.0f : dy[r * C + c];
        const float xh = (x[r * C + c] - m) * rs, dh = dyv * g[c];
        s1 += dh;
        s2 = fmaf(dh, xh, s2);
    }
    s1 = wave_sum(s1) / (float)C;
    s2 = wave_sum(s2) / (float)C;
    for (int c = lane; c < C; c += 64) {
        const float dyv = (y_relu && !relu_passes(y_relu[r * C + c])) ? 0.0f : dy[r * C + c];
        const float xv = x[r * C + c], xh = (xv - m) * rs, dh = dyv * g[c];
        dx[r * C + c] = rs * (dh - s1 - xh * s2) * act_grad_from_output(in_act, xv);
    }
}
// The epilogue of the two kernels below: red[wave][dgamma | dbeta][256] holds every wave's sums over its rows; the four waves' are
// added in wave order (fixed: reproducible) -> out[dg (C) | db (C)], the workgroup's partial row
__device__ __forceinline__ void ln_param_partials(const float* red, int C, float* out) {
    __syncthreads();
    for (int e = (int)threadIdx.x; e < 2 * C; e += 256) {      // e < C: dgamma[e], else dbeta[e - C]
        const int which = e >= C ? 1 : 0, c = e - which * C;
        out[e] = ((red[(0 * 2 + which) * 256 + c] + red[(1 * 2 + which) * 256 + c]) + red[(2 * 2 + which) * 256 + c]) +
                 red[(3 * 2 + which) * 256 + c];
    }
}
// dx and the parameter-gradient partials in one pass (C <= 256): a 4-wave workgroup per kLnRows rows, one wave per quarter, lanes
// across the channels; every lane keeps dgamma / dbeta sums of its (up to four) channels over its wave's rows, the four waves'
// sums are added in wave order through LDS -> partial[workgroup][dg (C) | db (C)]
constexpr int kLnRows = 64;
static __global__ __launch_bounds__(256) void train_ln_bwd_fused_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ dy, long rows, int C,
                                                                 float* __restrict__ dx, float* __restrict__ partial,
                                                                 const unsigned char* __restrict__ rowmask, int in_act,
                                                                 const float* __restrict__ y_relu) {
    ESMI_DYN_LDS(red);   // [4 waves][2][256] floats
    const long chunk = blockIdx.x;
    const int lane = lane_id(), w = wave_id();
    // this wave's quarter of the workgroup's rows
    const ChunkRange cr = chunk_range(chunk * 4 + w, kLnRows / 4, chunk_range(chunk, kLnRows, rows).r1);
    float gg[4], dga[4] = {0.f, 0.f, 0.f, 0.f}, dba[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u) gg[u] = lane + 64 * u < C ? g[lane + 64 * u] : 0.0f;
    for (long r = cr.r0; r < cr.r1; ++r) {
        const float m = mean[r], rs = rstd[r];
        const bool masked = rowmask && rowmask[r];   // (a zero dy row: dx = 0, no contribution to dgamma / dbeta)
        float xv[4], xh[4], dh[4], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = lane + 64 * u;
            const bool ok = c < C;
            const float d = (ok && !masked && !(y_relu && !relu_passes(y_relu[r * C + c]))) ? dy[r * C + c] : 0.0f;
            xv[u] = ok ? x[r * C + c] : 0.0f;
            xh[u] = ok ? (xv[u] - m) * rs : 0.0f;
            dh[u] = d * gg[u];
            s1 += dh[u];
            s2 = fmaf(dh[u], xh[u], s2);
            dga[u] = fmaf(d, xh[u], dga[u]);
            dba[u] += d;
        }
        s1 = wave_sum(s1) / (float)C;
        s2 = wave_sum(s2) / (float)C;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = lane + 64 * u;
            if (c < C) dx[r * C + c] = rs * (dh[u] - s1 - xh[u] * s2) * act_grad_from_output(in_act, xv[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        red[(w * 2 + 0) * 256 + lane + 64 * u] = dga[u];
        red[(w * 2 + 1) * 256 + lane + 64 * u] = dba[u];
    }
    ln_param_partials(red, C, partial + chunk * 2 * C);
}

// The same for C = 4 LPR in {32, 64, 128} on 16-byte aligned tensors (round 5): LPR lanes per row, 64 / LPR rows per pass, 16-byte
// accesses, and ALL of a wave's 16 rows loaded before the first is used -- the kernel above walks its rows one by one, every row a
// dependent round trip (mean, rstd, mask, then x and dy): 20 us for an encoder-size launch of 1.6 MB, 29 us at decoder size.  A lane's
// dgamma / dbeta sums run over the rows of its lane group; the groups are then added by a fixed butterfly, the waves in wave order.
template <int LPR>
static __global__ __launch_bounds__(256) void train_ln_bwd4_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ dy, long rows, float* __restrict__ dx,
                                                            float* __restrict__ partial, const unsigned char* __restrict__ rowmask,
                                                            int in_act, const float* __restrict__ y_relu) {
    constexpr int RPW = 64 / LPR, C = 4 * LPR, WROWS = kLnRows / 4, NP = WROWS / RPW;
    ESMI_DYN_LDS(red);   // [4 waves][2][256] floats
    const long chunk = blockIdx.x;
    const int lane = lane_id(), w = wave_id(), sub = lane / LPR, l = lane % LPR;
    const long rw0 = chunk * kLnRows + (long)w * WROWS + sub;          // this lane's row of pass p: rw0 + RPW p
    const f32x4 gv = ld4(g + 4 * l);
    f32x4 xv[NP], dv[NP];
    float mm[NP], rr[NP];
    unsigned livem = 0u, maskm = 0u;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const long r = rw0 + RPW * p, rc = r < rows ? r : rows - 1;
        xv[p] = ld4(x + rc * C + 4 * l);
        dv[p] = ld4(dy + rc * C + 4 * l);
        mm[p] = mean[rc];
        rr[p] = rstd[rc];
        if (r < rows) livem |= 1u << p;
    }
    if (rowmask) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const long r = rw0 + RPW * p;
            if (rowmask[r < rows ? r : rows - 1]) maskm |= 1u << p;
        }
    }
    if (y_relu) {   // dy counts only where the forward's relu(LN(.)) output is positive
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const long r = rw0 + RPW * p;
            const f32x4 yv = ld4(y_relu + (r < rows ? r : rows - 1) * C + 4 * l);
#pragma unroll
            for (int e = 0; e < 4; ++e) if (!relu_passes(yv[e])) dv[p][e] = 0.0f;
        }
    }
    f32x4 dga = zero4(), dba = zero4();
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const bool live = (livem >> p) & 1u;
        if (!live || ((maskm >> p) & 1u)) dv[p] = zero4();            // (a zero dy row: dx = 0, no contribution to dgamma / dbeta)
        f32x4 xh, dh;
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xh[e] = (xv[p][e] - mm[p]) * rr[p];
            dh[e] = dv[p][e] * gv[e];
            s1 += dh[e];
            s2 = fmaf(dh[e], xh[e], s2);
            dga[e] = fmaf(dv[p][e], xh[e], dga[e]);
            dba[e] += dv[p][e];
        }
        s1 = group_sum<LPR>(s1) / (float)C;
        s2 = group_sum<LPR>(s2) / (float)C;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rr[p] * (dh[e] - s1 - xh[e] * s2) * act_grad_from_output(in_act, xv[p][e]);
        if (live) *reinterpret_cast<f32x4*>(dx + (rw0 + RPW * p) * C + 4 * l) = o;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        dga[e] = across_groups_sum<LPR>(dga[e]);
        dba[e] = across_groups_sum<LPR>(dba[e]);
    }
    if (sub == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[(w * 2 + 0) * 256 + 4 * l + e] = dga[e];
            red[(w * 2 + 1) * 256 + 4 * l + e] = dba[e];
        }
    }
    ln_param_partials(red, C, partial + chunk * 2 * C);
}

// partial[chunk][0][c] = sum dy * xhat, partial[chunk][1][c] = sum dy over the chunk's rows
static __global__ void train_ln_bwd_params_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                           const float* __restrict__ dy, long rows, int C, float* __restrict__ partial,
                                           const unsigned char* __restrict__ rowmask, const float* __restrict__ y_relu) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= C) return;
    const ChunkRange cr = chunk_range(blockIdx.y, kTrainChunk, rows);
    float a = 0.0f, s = 0.0f;
    for (long r = cr.r0; r < cr.r1; ++r) {
        const float d = ((rowmask && rowmask[r]) || (y_relu && !relu_passes(y_relu[r * C + c]))) ? 0.0f : dy[r * C + c];
        a = fmaf(d, (x[r * C + c] - mean[r]) * rstd[r], a);
        s += d;
    }
    partial[(long)blockIdx.y * 2 * C + c] = a;
    partial[(long)blockIdx.y * 2 * C + C + c] = s;
}

// ---- activations: kind as esmi_dev.h Act (1 ReLU, 2 GELU erf, 3 tanh); backward reads y for ReLU / tanh and x for GELU
static __global__ void train_act_fwd_kernel(const float* __restrict__ x, long n, int kind, float* __restrict__ y) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float v = x[q];
    y[q] = kind == ACT_RELU ? fmaxf(v, 0.0f) : (kind == ACT_GELU ? 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)) : tanhf(v));
}
static __global__ void train_act_bwd_kernel(const float* __restrict__ saved, const float* __restrict__ dy, long n, int kind,
                                     float* __restrict__ dx) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float s = saved[q];
    float d;
    if (kind == ACT_RELU) d = s > 0.0f ? 1.0f : 0.0f;
    else if (kind == ACT_TANH) d = 1.0f - s * s;
    else d = 0.5f * (1.0f + erff(s * 0.70710678118654752f)) + s * 0.3989422804014327f * expf(-0.5f * s * s);
    dx[q] = dy[q] * d;
}

}  // namespace esmi
