// Training step: the operators around the sequence -- embedding, row masking, residual add, column-block copies and torch.cat,
// the length regulator.  One thread per output element (the embedding's backward: per table element and chunk of rows, the first
// stage of a two-stage reduction, train_reduce.h).
#pragma once
#include "train_reduce.h"

namespace esmi {

// ---- embedding: forward gather (out-of-range ids read row 0); backward one thread per table element, rows with id ==
// padding_idx get no gradient (nn.Embedding(padding_idx), networks.py:32)
static __global__ void train_embed_fwd_kernel(const int* __restrict__ ids, const float* __restrict__ table, long rows, int V, int C,
                                       float* __restrict__ out) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= rows * C) return;
    int id = ids[q / C];
    if (id < 0 || id >= V) id = 0;
    out[q] = table[(long)id * C + q % C];
}
// (blockDim = 64.)  The chunk's ids come in by coalesced loads, 64 at a time; one ballot per vocabulary entry of the wave (its 64
// consecutive (v, c) elements span 64 / C + 1 entries at most) gives every lane the bit mask of ITS entry's rows, and the lane then
// visits only those, in row order: the same sums in the same order as a compare per (element, row) -- which read ids[r] through the
// scalar cache once per row (256 dependent ~200 ns loads per thread: 59 us for the phoneme table at B = 128).
static __global__ __launch_bounds__(64) void train_embed_bwd_kernel(const int* __restrict__ ids, const float* __restrict__ dy, long rows, int V, int C,
                                       int padding_idx, float* __restrict__ partial) {
    const long q0 = (long)blockIdx.x * 64, q = q0 + threadIdx.x;   // partial[chunk][v][c] over the chunk's rows
    const long nq = (long)V * C;
    const bool live = q < nq;
    const int v = live ? (int)(q / C) : -1, c = live ? (int)(q % C) : 0, lane = lane_id();
    const bool take = live && v != padding_idx;
    const long qe = q0 + 63 < nq ? q0 + 63 : nq - 1;
    const int v_lo = (int)(q0 / C), v_hi = (int)(qe / C);           // wave-uniform
    const ChunkRange cr = chunk_range(blockIdx.y, kTrainChunk, rows);
    const long r1 = cr.r1;
    float acc = 0.0f;
    for (long base = cr.r0; base < r1; base += 64) {
        const int idv = base + lane < r1 ? ids[base + lane] : -1;
        unsigned long long mine = 0ull;
        for (int vv = v_lo; vv <= v_hi; ++vv) {
            const unsigned long long m = ballot64(idv == vv);
            if (vv == v) mine = m;
        }
        if (!take) mine = 0ull;
        while (mine) {                                              // ascending rows
            const int rr = __builtin_ctzll(mine);
            mine &= mine - 1;
            acc += dy[(base + rr) * C + c];
        }
    }
    if (live) partial[(long)blockIdx.y * nq + q] = acc;
}

// ---- row masking (masked_fill(mask, 0) with a per-row mask), residual add, column-block copy (torch.cat / its gradient)
static __global__ void train_mask_rows_kernel(const float* __restrict__ x, const unsigned char* __restrict__ mask, long rows, int C,
                                       float* __restrict__ y) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= rows * C) return;
    y[q] = mask[q / C] ? 0.0f : x[q];
}
static __global__ void train_add_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, float* __restrict__ y) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) y[q] = a[q] + b[q];
}
static __global__ void train_copy_cols_kernel(const float* __restrict__ src, int ld_src, int col_src, float* __restrict__ dst, int ld_dst,
                                       int col_dst, long rows, int C) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= rows * C) return;
    const long r = q / C;
    const int c = (int)(q % C);
    dst[r * ld_dst + col_dst + c] = src[r * ld_src + col_src + c];
}

// torch.cat(parts, dim=-1) of up to 8 row-major parts in ONE launch, or its backward (the slices of dcat back into the parts);
// parts whose bit is set in `masked` are taken as zero on rows with rowmask[r] != 0 (x.masked_fill(mask, 0) before the cat,
// networks.py:366-368) -- the same mask zeroes those rows of their gradient
struct CatArgs { float* part[8]; int width[8]; int col[8]; int n, tot; long rows; float* cat; const unsigned char* rowmask; unsigned masked; int backward; };
static __global__ void train_cat_kernel(const CatArgs a) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.rows * a.tot) return;
    const long r = q / a.tot;
    const int c = (int)(q - r * a.tot);
    int pi = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j) pi += (j < a.n && c >= a.col[j]) ? 1 : 0;
    float* part = a.part[0];
    int w = a.width[0], c0 = a.col[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) if (pi == j) { part = a.part[j]; w = a.width[j]; c0 = a.col[j]; }
    const bool zero = ((a.masked >> pi) & 1u) && a.rowmask && a.rowmask[r];
    if (a.backward) part[r * w + (c - c0)] = zero ? 0.0f : a.cat[q];
    else a.cat[q] = zero ? 0.0f : part[r * w + (c - c0)];
}

// ---- length regulator (networks.py:233-244) forward / backward on the inclusive duration cumsum `cum` (B, T):
// frame f of utterance b copies phoneme t with cum[t-1] <= f < cum[t]; frames >= cum[T-1] are zero padding
static __global__ void train_repeat_fwd_kernel(const float* __restrict__ feat, const int* __restrict__ cum, int B, int T, int C, int L,
                                        float* __restrict__ out) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)B * L * C) return;
    const int c = (int)(q % C), f = (int)((q / C) % L), b = (int)(q / ((long)C * L));
    const int* cb = cum + (long)b * T;
    int lo = 0, hi = T;                       // first t with cum[t] > f
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cb[mid] > f) hi = mid; else lo = mid + 1; }
    out[q] = lo < T ? feat[((long)b * T + lo) * C + c] : 0.0f;
}
// the same, four channels per thread (C % 4 == 0, 16-byte aligned tensors, B L C / 4 < 2^31): one search per 16 bytes instead of one per float
static __global__ void train_repeat_fwd4_kernel(const float* __restrict__ feat, const int* __restrict__ cum, int B, int T, int C4, int L,
                                         float* __restrict__ out) {
    const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (unsigned)B * (unsigned)L * (unsigned)C4) return;
    const unsigned row = q / (unsigned)C4, c4 = q - row * (unsigned)C4, b = row / (unsigned)L, f = row - b * (unsigned)L;
    const int* cb = cum + (long)b * T;
    int lo = 0, hi = T;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cb[mid] > (int)f) hi = mid; else lo = mid + 1; }
    f32x4 v = zero4();
    if (lo < T) v = ld4(feat + (((long)b * T + lo) * C4 + c4) * 4);
    *reinterpret_cast<f32x4*>(out + (long)q * 4) = v;
}
static __global__ void train_repeat_bwd_kernel(const float* __restrict__ dout, const int* __restrict__ cum, int B, int T, int C, int L,
                                        float* __restrict__ dfeat) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)B * T * C) return;
    const int c = (int)(q % C), t = (int)((q / C) % T), b = (int)(q / ((long)C * T));
    const int f0 = t ? cum[(long)b * T + t - 1] : 0;
    int f1 = cum[(long)b * T + t];
    f1 = f1 < L ? f1 : L;
    float acc = 0.0f;
    for (int f = f0; f < f1; ++f) acc += dout[((long)b * L + f) * C + c];
    dfeat[q] = acc;
}

}  // namespace esmi
