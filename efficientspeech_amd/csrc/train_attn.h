// Training step: the attention core, blocks.py:43-64 (scores are NOT masked there): qkv (B, N, 3, h, C) -> P (B, h, N, N),
// ctx (B, N, h*C), and its backward in a row pass and a column pass.  A wave per query row: the lanes share the keys for the scores
// (wave reductions for max / sum in a fixed butterfly order, train_reduce.h), then the channels for the context row.
#pragma once
#include "train_reduce.h"

namespace esmi {

// One 64-thread workgroup per (b, head, query row), K and V read from global memory
static __global__ __launch_bounds__(64) void train_attn_fwd_kernel(const float* __restrict__ qkv, int B, int N, int C, int h, float scale,
                                                            float* __restrict__ P, float* __restrict__ ctx) {
    const long q = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int i = (int)(q % N), hd = (int)((q / N) % h), b = (int)(q / ((long)N * h));
    const long ld = 3L * h * C;
    const float* qi = qkv + ((long)b * N + i) * ld + (long)hd * C;
    float* p = P + (((long)b * h + hd) * N + i) * N;
    float mx = -3.0e38f;
    for (int j = lane; j < N; j += 64) {
        const float* kj = qkv + ((long)b * N + j) * ld + (long)(h + hd) * C;
        float s = 0.0f;
        for (int c = 0; c < C; ++c) s = fmaf(qi[c], kj[c], s);
        s *= scale;
        p[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.0f;
    for (int j = lane; j < N; j += 64) { const float e = expf(p[j] - mx); p[j] = e; sum += e; }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    for (int j = lane; j < N; j += 64) p[j] *= inv;
    __syncthreads();                                   // the row of P is complete for every lane
    float* o = ctx + ((long)b * N + i) * h * C + (long)hd * C;
    for (int c = lane; c < C; c += 64) {
        float a = 0.0f;
        for (int j = 0; j < N; ++j) a = fmaf(p[j], qkv[((long)b * N + j) * ld + (long)(2 * h + hd) * C + c], a);
        o[c] = a;
    }
}
// row i: dP = dctx_i . V^T, dS = P o (dP - <P, dP>), dq_i = scale dS K;  dS (B, h, N, N) kept for the column pass
static __global__ __launch_bounds__(64) void train_attn_bwd_rows_kernel(const float* __restrict__ qkv, const float* __restrict__ P,
                                                                 const float* __restrict__ dctx, int B, int N, int C, int h,
                                                                 float scale, float* __restrict__ dS, float* __restrict__ dqkv) {
    const long q = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const int i = (int)(q % N), hd = (int)((q / N) % h), b = (int)(q / ((long)N * h));
    const long ld = 3L * h * C;
    const float* p = P + (((long)b * h + hd) * N + i) * N;
    float* ds = dS + (((long)b * h + hd) * N + i) * N;
    const float* go = dctx + ((long)b * N + i) * h * C + (long)hd * C;
    float dot = 0.0f;
    for (int j = lane; j < N; j += 64) {
        const float* vj = qkv + ((long)b * N + j) * ld + (long)(2 * h + hd) * C;
        float a = 0.0f;
        for (int c = 0; c < C; ++c) a = fmaf(go[c], vj[c], a);
        ds[j] = a;
        dot = fmaf(p[j], a, dot);
    }
    dot = wave_sum(dot);
    for (int j = lane; j < N; j += 64) ds[j] = p[j] * (ds[j] - dot);
    __syncthreads();
    float* dq = dqkv + ((long)b * N + i) * ld + (long)hd * C;
    for (int c = lane; c < C; c += 64) {
        float a = 0.0f;
        for (int j = 0; j < N; ++j) a = fmaf(ds[j], qkv[((long)b * N + j) * ld + (long)(h + hd) * C + c], a);
        dq[c] = a * scale;
    }
}
// The same two kernels with the head's K and V staged once in LDS ([N][C + 1] each: a lane per key reads its row at an odd
// stride, a lane per channel reads consecutive words -- both conflict-free), one 256-thread workgroup per (b, head), every wave
// taking query rows w, w + 4, ...  Used whenever 2 N (C + 1) + 4 N floats fit (tiny / small ES at any realistic length); the
// global-memory versions above remain for the rest.
__host__ __device__ inline size_t train_attn_lds_bytes(int N, int C) { return ((size_t)2 * N * (C + 1) + 4 * (size_t)N) * sizeof(float); }
// the LDS of both kernels: K [N][C + 1] | V [N][C + 1] | one row of N floats per wave.  attn_stage_kv fills K and V of (b, head hd)
// with the whole workgroup and returns behind the barrier.
struct AttnLds { float *Ks, *Vs, *row; };
__device__ __forceinline__ AttnLds attn_stage_kv(float* lds, const float* qkv, int b, int hd, int N, int C, int h) {
    const AttnLds s = {lds, lds + (long)N * (C + 1), lds + 2 * (long)N * (C + 1) + (long)wave_id() * N};
    const long ld = 3L * h * C;
    for (int e = (int)threadIdx.x; e < N * C; e += 256) {
        const int j = e / C, c = e - j * C;
        s.Ks[j * (C + 1) + c] = qkv[((long)b * N + j) * ld + (long)(h + hd) * C + c];
        s.Vs[j * (C + 1) + c] = qkv[((long)b * N + j) * ld + (long)(2 * h + hd) * C + c];
    }
    __syncthreads();
    return s;
}
// gridDim.y row segments per (utterance, head): B * h workgroups alone leave most of the chip idle at the reference's batch size.
// Query rows [lo, hi) of this workgroup's segment.
struct AttnRows { int lo, hi; };
__device__ __forceinline__ AttnRows attn_row_segment(int N) {
    const int seg = (N + (int)gridDim.y - 1) / (int)gridDim.y, lo = (int)blockIdx.y * seg;
    return {lo, lo + seg < N ? lo + seg : N};
}
static __global__ __launch_bounds__(256) void train_attn_fwd_lds_kernel(const float* __restrict__ qkv, int B, int N, int C, int h, float scale,
                                                                 float* __restrict__ P, float* __restrict__ ctx) {
    ESMI_DYN_LDS(lds);
    const int hd = (int)(blockIdx.x % h), b = (int)(blockIdx.x / h), lane = lane_id(), w = wave_id();
    const long ld = 3L * h * C;
    const AttnLds kv = attn_stage_kv(lds, qkv, b, hd, N, C, h);
    const float *Ks = kv.Ks, *Vs = kv.Vs;
    float* prow = kv.row;                               // this wave's softmax row
    const AttnRows rows = attn_row_segment(N);
    for (int i = rows.lo + w; i < rows.hi; i += 4) {
        const float* qi = qkv + ((long)b * N + i) * ld + (long)hd * C;
        float* p = P + (((long)b * h + hd) * N + i) * N;
        float mx = -3.0e38f;
        for (int j = lane; j < N; j += 64) {
            float s = 0.0f;
            for (int c = 0; c < C; ++c) s = fmaf(qi[c], Ks[j * (C + 1) + c], s);
            s *= scale;
            prow[j] = s;
            mx = fmaxf(mx, s);
        }
        mx = wave_max(mx);
        float sum = 0.0f;
        for (int j = lane; j < N; j += 64) { const float e = expf(prow[j] - mx); prow[j] = e; sum += e; }
        sum = wave_sum(sum);
        const float inv = 1.0f / sum;
        for (int j = lane; j < N; j += 64) { const float v = prow[j] * inv; prow[j] = v; p[j] = v; }
        lds_wave_sync();                               // the row is read back by other lanes of this wave
        float* o = ctx + ((long)b * N + i) * h * C + (long)hd * C;
        for (int c = lane; c < C; c += 64) {
            float a = 0.0f;
            for (int j = 0; j < N; ++j) a = fmaf(prow[j], Vs[j * (C + 1) + c], a);
            o[c] = a;
        }
        lds_wave_sync();                               // before the next row overwrites prow
    }
}
static __global__ __launch_bounds__(256) void train_attn_bwd_rows_lds_kernel(const float* __restrict__ qkv, const float* __restrict__ P,
                                                                      const float* __restrict__ dctx, int B, int N, int C, int h,
                                                                      float scale, float* __restrict__ dS, float* __restrict__ dqkv) {
    ESMI_DYN_LDS(lds);
    const int hd = (int)(blockIdx.x % h), b = (int)(blockIdx.x / h), lane = lane_id(), w = wave_id();
    const long ld = 3L * h * C;
    const AttnLds kv = attn_stage_kv(lds, qkv, b, hd, N, C, h);
    const float *Ks = kv.Ks, *Vs = kv.Vs;
    float* drow = kv.row;                               // this wave's row of dS
    const AttnRows rows = attn_row_segment(N);
    for (int i = rows.lo + w; i < rows.hi; i += 4) {
        const float* p = P + (((long)b * h + hd) * N + i) * N;
        float* ds = dS + (((long)b * h + hd) * N + i) * N;
        const float* go = dctx + ((long)b * N + i) * h * C + (long)hd * C;
        float dot = 0.0f;
        for (int j = lane; j < N; j += 64) {
            float a = 0.0f;
            for (int c = 0; c < C; ++c) a = fmaf(go[c], Vs[j * (C + 1) + c], a);
            drow[j] = a;
            dot = fmaf(p[j], a, dot);
        }
        dot = wave_sum(dot);
        for (int j = lane; j < N; j += 64) { const float v = p[j] * (drow[j] - dot); drow[j] = v; ds[j] = v; }
        lds_wave_sync();
        float* dq = dqkv + ((long)b * N + i) * ld + (long)hd * C;
        for (int c = lane; c < C; c += 64) {
            float a = 0.0f;
            for (int j = 0; j < N; ++j) a = fmaf(drow[j], Ks[j * (C + 1) + c], a);
            dq[c] = a * scale;
        }
        lds_wave_sync();
    }
}

// column j, channel c: dk_j = scale dS^T Q, dv_j = P^T dctx   (one thread per (b, head, j, c))
static __global__ void train_attn_bwd_cols_kernel(const float* __restrict__ qkv, const float* __restrict__ P, const float* __restrict__ dS,
                                           const float* __restrict__ dctx, int B, int N, int C, int h, float scale,
                                           float* __restrict__ dqkv) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)B * h * N * C) return;
    const int c = (int)(q % C), j = (int)((q / C) % N), hd = (int)((q / ((long)C * N)) % h), b = (int)(q / ((long)C * N * h));
    const long ld = 3L * h * C;
    float a = 0.0f, v = 0.0f;
    for (int i = 0; i < N; ++i) {
        const long pi = (((long)b * h + hd) * N + i) * N + j;
        a = fmaf(dS[pi], qkv[((long)b * N + i) * ld + (long)hd * C + c], a);
        v = fmaf(P[pi], dctx[((long)b * N + i) * h * C + (long)hd * C + c], v);
    }
    dqkv[((long)b * N + j) * ld + (long)(h + hd) * C + c] = a * scale;
    dqkv[((long)b * N + j) * ld + (long)(2 * h + hd) * C + c] = v;
}

}  // namespace esmi
