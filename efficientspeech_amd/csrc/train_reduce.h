// Training step: the reduction vocabulary every family header shares, and the second stage of the two-stage reductions.
// Every function here adds in a FIXED order (a butterfly over fixed lane distances, a tree over fixed strides, partials in chunk
// order), so whatever is built from them gives the same bits on every run (train_ops.h: the contract).
#pragma once
#include "esmi_dev.h"

namespace esmi {

// ---- inside a wave: xor butterflies.  Every lane ends up with the result.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += shfl_xor_f(v, m);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, shfl_xor_f(v, m));
    return v;
}
// a wave as 64 / LPR groups of LPR consecutive lanes (one row per group): the sum inside every group ...
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int k = LPR / 2; k > 0; k >>= 1) v += shfl_xor_f(v, k);
    return v;
}
// ... and, per lane position, the sum across the groups
template <int LPR>
__device__ __forceinline__ float across_groups_sum(float v) {
#pragma unroll
    for (int k = LPR; k < 64; k <<= 1) v += shfl_xor_f(v, k);
    return v;
}
// ---- inside a 256-thread workgroup: a tree through `red` (256 T); every thread gets the sum, and `red` is free again on return
template <class T>
__device__ __forceinline__ T block_sum_256(T v, T* red) {
    const int tid = (int)threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

// ---- over the rows (B * n positions), in two deterministic stages: stage 1 gives every (output element, chunk of kTrainChunk rows)
// its own thread and writes a partial sum, stage 2 adds the partials of an element in chunk order.
constexpr int kTrainChunk = 256;
__host__ __device__ inline long train_chunks(long rows, int chunk = kTrainChunk) { return (rows + chunk - 1) / chunk; }
// rows [r0, r1) of chunk `idx`
struct ChunkRange { long r0, r1; };
__device__ __forceinline__ ChunkRange chunk_range(long idx, long chunk, long rows) {
    const long r0 = idx * chunk;
    return {r0, r0 + chunk < rows ? r0 + chunk : rows};
}

// out[e] = sum over chunks of partial[chunk * stride + e], e < n.  64 elements x kReduceGroups interleaved chunk groups per
// workgroup; the group sums are added in group order (fixed order: reproducible).  (The CPU simulator build uses 4 groups and
// 8 loss workgroups: a fiber per thread makes 1024-thread workgroups the slowest thing in the test suite.)
// (kReduceGroups: wavesim_shim.h)
static __global__ __launch_bounds__(64 * kReduceGroups) void train_reduce_chunks_kernel(const float* __restrict__ partial, long n, long stride,
                                                                                long chunks, float* __restrict__ out,
                                                                                long n0 = -1, float* __restrict__ out1 = nullptr) {
    ESMI_DYN_LDS(red);   // 64 * kReduceGroups floats
    const int ex = (int)(threadIdx.x & 63), cy = (int)(threadIdx.x >> 6);
    const long q = (long)blockIdx.x * 64 + ex;
    float acc = 0.0f;
    if (q < n)
        for (long c = cy; c < chunks; c += kReduceGroups) acc += partial[c * stride + q];
    red[cy * 64 + ex] = acc;
    __syncthreads();
    if (cy == 0 && q < n) {
        float t = red[ex];
#pragma unroll
        for (int u = 1; u < kReduceGroups; ++u) t += red[u * 64 + ex];
        if (out1 && q >= n0) out1[q - n0] = t;      // second segment of a partial row (e.g. the bias sums after the weight sums)
        else out[q] = t;
    }
}
// the same for a batch of independent reductions in one launch: the queued second stages of a training step
struct ReduceItem { const float* partial; long n, stride, chunks; float* out; long n0; float* out1; };
constexpr int kReduceBatch = 48;
// (first[i]: the first workgroup of item i in the launch's 1-D grid, first[count]: the grid size.  A 2-D grid sized for the largest
// item launched ~14,700 workgroups of 16 waves for the step's 48 reductions, most of them leaving at once: 57 us, bound by the dispatcher.)
struct ReduceBatch { int count; int first[kReduceBatch + 1]; ReduceItem items[kReduceBatch]; };
static __global__ __launch_bounds__(64 * kReduceGroups) void train_reduce_batch_kernel(const ReduceBatch b) {
    ESMI_DYN_LDS(red);   // 64 * kReduceGroups floats
    int ii = 0;
    while (ii + 1 < b.count && (int)blockIdx.x >= b.first[ii + 1]) ++ii;     // (workgroup-uniform)
    const ReduceItem& it = b.items[ii];
    const int ex = (int)(threadIdx.x & 63), cy = (int)(threadIdx.x >> 6);
    const long q = (long)((int)blockIdx.x - b.first[ii]) * 64 + ex;
    float acc = 0.0f;
    if (q < it.n)
        for (long c = cy; c < it.chunks; c += 4 * kReduceGroups) {   // four loads in flight, added in chunk order (the loop was one exposed
            float v[4];                                               // round trip per partial row: 57 us for the step's 55 MB)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long cc = c + (long)u * kReduceGroups;
                v[u] = it.partial[(cc < it.chunks ? cc : c) * it.stride + q];
                if (cc >= it.chunks) v[u] = 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += v[u];
        }
    red[cy * 64 + ex] = acc;
    __syncthreads();
    if (cy == 0 && q < it.n) {
        float t = red[ex];
#pragma unroll
        for (int u = 1; u < kReduceGroups; ++u) t += red[u * 64 + ex];
        if (it.out1 && q >= it.n0) it.out1[q - it.n0] = t;
        else it.out[q] = t;
    }
}
// partial[chunk][c] = sum over the chunk's rows of v[row, c]   (bias gradients)
static __global__ void train_colsum_kernel(const float* __restrict__ v, long rows, int C, float* __restrict__ partial, long pstride, int chunk) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= C) return;
    const ChunkRange cr = chunk_range(blockIdx.y, chunk, rows);
    float acc = 0.0f;
    for (long r = cr.r0; r < cr.r1; ++r) acc += v[r * C + c];
    partial[(long)blockIdx.y * pstride + c] = acc;
}

}  // namespace esmi
