// Training step: weight gradients -- the first stage of the two-stage reduction over the rows (train_reduce.h).  Every kernel
// writes partial[chunk][weight element in checkpoint order] (and the bias partials behind them): one thread per weight element,
// the two depthwise kernels, the dense one on the matrix pipe, and the Linear down to one channel with its three gradients in one
// launch.
#pragma once
#include "train_conv.h"
#include "train_reduce.h"

namespace esmi {

constexpr int kTrainChunkDw = 128;     // rows per workgroup of the depthwise weight gradient (8 sub-chunks of 16 rows, summed in LDS; 256: 300 workgroups at B = 128, 38 us)
// (rows per wave of the matrix-pipe weight gradient: tu_train.hip wgrad_chunk -- a multiple of 16 sized for one round of workgroups.
// Round 3, when a trip was a chain of exposed load latencies, a fixed 48 ... 192 rows made no difference: 5.2-5.7 ms per B = 128 step.)

// dw(co, ci, j) = sum over (b, t) of dy[b, t, co] * x[b, in_pos(t, j), ci]: partial[chunk][weight element in checkpoint order]
static __global__ void train_conv_wgrad_kernel(const ConvDesc d, const float* __restrict__ x, const float* __restrict__ dy,
                                        float* __restrict__ partial, long pstride, int chunk) {
    const int cig = d.transposed ? d.c_out : d.c_in / d.groups;      // middle extent of the checkpoint layout
    const int outer = d.transposed ? d.c_in : d.c_out;
    const long nw = (long)outer * cig * d.k;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nw) return;
    const int j = (int)(q % d.k), mid = (int)((q / d.k) % cig), out = (int)(q / ((long)d.k * cig));
    int co, ci;
    if (d.transposed) { ci = out; co = mid; }
    else { co = out; ci = (co / (d.c_out / d.groups)) * cig + mid; }
    const ChunkRange cr = chunk_range(blockIdx.y, chunk, (long)d.B * d.n_out);
    float acc = 0.0f;
    for (long r = cr.r0; r < cr.r1; ++r) {
        const int b = (int)(r / d.n_out), t = (int)(r - (long)b * d.n_out);
        const int ti = conv_in_pos(d, t, j);
        if (ti < 0) continue;
        acc = fmaf(dy[r * d.c_out + co], x[((long)b * d.n_in + ti) * d.c_in + ci], acc);
    }
    partial[(long)blockIdx.y * pstride + q] = acc;
}
// A Linear down to ONE channel (the variance predictors' last layer, networks.py:162): its three gradients in one launch -- dx = dy w,
// and per chunk of <= 64 rows the partial sums of dw = sum_r dy[r] x[r, :] and db = sum_r dy[r] (row order / a fixed butterfly:
// reproducible).  One wave per chunk: lane l keeps dy of row l, the lanes then run across the channels (coalesced) with dy handed
// round by v_readlane.  (Before: data gradient, weight gradient and column sum as three launches, the weight gradient with a 64-bit
// division per row and thread: 5 + 20 + 5 us per predictor at B = 128.)
static __global__ __launch_bounds__(64) void train_lin1_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ w,
                                                            long rows, int C, float* __restrict__ dx, float* __restrict__ partial,
                                                            float* __restrict__ partial_bias, long pstride, int chunk) {
    const int lane = lane_id();
    const ChunkRange cr = chunk_range(blockIdx.x, chunk, rows);
    const long r0 = cr.r0;
    const int nr = (int)(cr.r1 - cr.r0);
    const float dyv = lane < nr ? dy[r0 + lane] : 0.0f;
    const int dyb = __builtin_bit_cast(int, dyv);
    for (int c0 = 0; c0 < C; c0 += 64) {               // (every lane runs the loop: the hand-round is a wave-level exchange)
        const int c = c0 + lane;
        const bool ok = c < C;
        const float wc = ok ? w[c] : 0.0f;
        float acc = 0.0f;
#pragma unroll 8
        for (int rr = 0; rr < nr; ++rr) {
            const float g = __builtin_bit_cast(float, bcast_i(dyb, rr));
            if (ok) {
                acc = fmaf(g, x[(r0 + rr) * C + c], acc);
                dx[(r0 + rr) * C + c] = g * wc;
            }
        }
        if (ok) partial[(long)blockIdx.x * pstride + c] = acc;
    }
    if (partial_bias) {
        const float t = wave_sum(dyv);
        if (lane == 0) partial_bias[(long)blockIdx.x * pstride] = t;
    }
}
// The same for C = 4 LPR in {16 .. 256} on 16-byte aligned tensors and a chunk of 32 rows: LPR lanes per row, 64 / LPR rows per pass,
// 16-byte accesses, every load of the chunk in flight before the first use; the lane groups' sums are added by a fixed butterfly.
template <int LPR>
static __global__ __launch_bounds__(64) void train_lin1_bwd4_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ w,
                                                             long rows, float* __restrict__ dx, float* __restrict__ partial,
                                                             float* __restrict__ partial_bias, long pstride) {
    constexpr int RPW = 64 / LPR, C = 4 * LPR, CH = 32, NP = CH / RPW;
    const int lane = lane_id(), sub = lane / LPR, l = lane % LPR;
    const long r0 = (long)blockIdx.x * CH + sub;                       // this lane's row of pass p: r0 + RPW p
    const f32x4 wv = ld4(w + 4 * l);
    f32x4 xv[NP];
    float g[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const long r = r0 + RPW * p, rc = r < rows ? r : rows - 1;
        xv[p] = ld4(x + rc * C + 4 * l);
        g[p] = r < rows ? dy[rc] : 0.0f;
    }
    f32x4 acc = zero4();
    float gs = 0.0f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const long r = r0 + RPW * p;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { acc[e] = fmaf(g[p], xv[p][e], acc[e]); o[e] = g[p] * wv[e]; }
        gs += g[p];
        if (r < rows) *reinterpret_cast<f32x4*>(dx + r * C + 4 * l) = o;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = across_groups_sum<LPR>(acc[e]);
    gs = across_groups_sum<LPR>(gs);
    if (sub == 0) {                                   // (pstride = C + 1: the partial rows are not 16-byte aligned)
#pragma unroll
        for (int e = 0; e < 4; ++e) partial[(long)blockIdx.x * pstride + 4 * l + e] = acc[e];
    }
    if (partial_bias && lane == 0) partial_bias[(long)blockIdx.x * pstride] = gs;
}
// depthwise (groups == C, one input channel per output channel, k <= 8): lanes across the channels (coalesced), every thread
// keeps the k tap sums and the bias sum of its channel over the chunk's rows
static __global__ void train_conv_wgrad_dw_kernel(const ConvDesc d, const float* __restrict__ x, const float* __restrict__ dy,
                                           float* __restrict__ partial, float* __restrict__ partial_bias, long pstride) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= d.c_out) return;
    const ChunkRange cr = chunk_range(blockIdx.y, kTrainChunkDw, (long)d.B * d.n_out);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bs = 0.0f;
    for (long r = cr.r0; r < cr.r1; ++r) {
        const int b = (int)(r / d.n_out), t = (int)(r - (long)b * d.n_out);
        const float g = dy[r * d.c_out + c];
        bs += g;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j >= d.k) break;
            const int ti = conv_in_pos(d, t, j);
            if (ti >= 0) acc[j] = fmaf(g, x[((long)b * d.n_in + ti) * d.c_in + c], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < d.k) partial[(long)blockIdx.y * pstride + (long)c * d.k + j] = acc[j];
    if (partial_bias) partial_bias[(long)blockIdx.y * pstride + c] = bs;
}

// The same for C % 4 == 0, stride 1, n_in == n_out (every depthwise convolution of the model): a 256-thread workgroup = 32 channel
// quads x kDwSub row sub-chunks of one chunk.  A thread walks its kTrainChunkDw / kDwSub rows in groups of 8: 8 rows of dY and 8 + k - 1 rows of X
// (16-byte loads; the input row of tap j for flat row r is flat row r + j - pad) feed 8 k fused multiply-adds per channel -- 2.5 loads
// per row instead of 6 scalar ones; a group that touches an utterance edge takes the tap-by-tap path.  The sub-chunks' sums are
// added in LDS in sub-chunk order (fixed: reproducible) and one partial row per workgroup goes out.
constexpr int kDwSub = 8;
static __global__ __launch_bounds__(256) void train_conv_wgrad_dw4_kernel(const ConvDesc d, const float* __restrict__ x, const float* __restrict__ dy,
                                                                   float* __restrict__ partial, float* __restrict__ partial_bias, long pstride) {
    ESMI_DYN_LDS(red);   // [kDwSub][9][128]: sub-chunk, tap (8 = bias), channel within the workgroup's 128
    const int lq = (int)threadIdx.x & 31, sub = (int)threadIdx.x >> 5;
    const int c = ((int)blockIdx.x * 32 + lq) * 4;
    const long rows = (long)d.B * d.n_out;
    const ChunkRange cr = chunk_range((long)blockIdx.y * kDwSub + sub, kTrainChunkDw / kDwSub, rows);   // this thread's sub-chunk
    const long c0 = cr.r0, c1 = cr.r1;
    f32x4 acc[8], bs = zero4();
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = zero4();
    if (c < d.c_out) {
        const int n = d.n_out, reach = d.k - 1 - d.pad;
        for (long g0 = c0; g0 < c1; g0 += 8) {
            const int t0 = (int)(g0 % n);
            // every load of the group first, unconditionally (rows clamped into the tensor; what must not count is masked below).  Round 5:
            // a group that touched an utterance edge took a tap-by-tap path of ~40 dependent loads, and one such lane held its whole wave --
            // a tenth of the waves ran ~20x longer than the rest (38 us per launch at B = 128 for 78 MB).
            f32x4 v[15], g[8];
#pragma unroll
            for (int r = 0; r < 15; ++r) {
                long xr = g0 - d.pad + r;
                xr = xr < 0 ? 0 : (xr >= rows ? rows - 1 : xr);
                v[r] = r < 8 + d.k - 1 ? ld4(x + xr * d.c_in + c) : zero4();
            }
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                const bool ok = g0 + o < c1;
                g[o] = ld4(dy + (ok ? g0 + o : c1 - 1) * d.c_out + c);
                if (!ok) g[o] = zero4();
                bs += g[o];
            }
            if (g0 + 8 <= c1 && t0 >= d.pad && t0 + 7 + reach < n) {     // the whole group and all its taps inside one utterance
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (j >= d.k) break;
#pragma unroll
                    for (int o = 0; o < 8; ++o)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(g[o][e], v[o + j][e], acc[j][e]);
                }
            } else {                                                      // an utterance edge inside the group: the same sums, tap by tap masked
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (j >= d.k) break;
#pragma unroll
                    for (int o = 0; o < 8; ++o) {
                        const int ti = (t0 + o) % n + j - d.pad;              // (the row's own utterance: rows past the chunk have g = 0)
                        const bool ok = ti >= 0 && ti < n;
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(g[o][e], ok ? v[o + j][e] : 0.0f, acc[j][e]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(red + ((sub * 9 + j) * 32 + lq) * 4) = acc[j];
    *reinterpret_cast<f32x4*>(red + ((sub * 9 + 8) * 32 + lq) * 4) = bs;
    __syncthreads();
    // thread -> (tap or bias, channel): 9 x 128 sums over the 8 sub-chunks
    for (int q = (int)threadIdx.x; q < 9 * 128; q += 256) {
        const int j = q >> 7, cc = q & 127, ch = (int)blockIdx.x * 128 + cc;
        if (ch >= d.c_out || (j < 8 && j >= d.k)) continue;
        float sum = 0.0f;
#pragma unroll
        for (int s2 = 0; s2 < kDwSub; ++s2) sum += red[(s2 * 9 + j) * 128 + cc];
        if (j < 8) partial[(long)blockIdx.y * pstride + (long)ch * d.k + j] = sum;
        else if (partial_bias) partial_bias[(long)blockIdx.y * pstride + ch] = sum;
    }
}

// The same partial sums for DENSE convolutions on the matrix pipe: dW_j = dY^T X_j is a GEMM with the rows as the contraction
// (v_mfma_f32_32x32x2_f32: exact fp32 products, k-ordered accumulation).  One wave = a block of 128 output channels x one
// 32-channel input tile x one tap x one chunk of rows.  Lane (i, kh) reads 16 bytes of dY -- channels 4i..4i+3 of row r + kh,
// so the 32 lanes of a half cover the whole 128-channel block, fully coalesced -- and one float of X; the four values feed four
// MFMAs whose tiles are the channel sets {4m + t}: four MFMAs per two loads, dY read once per input tile instead of once per
// (input tile, output tile).  The (tap 0, first input tile) waves also sum dY's columns: the bias gradient.
constexpr int kWgradWaves = 4;                      // waves (= row chunks) per workgroup, summed in LDS before anything is written
constexpr int kWgradLdsBytes = kWgradWaves * 64 * 64 * 4;   // [wave][accumulator register 0..63][lane]
// One trip's loads of the ConvTranspose1d weight gradient (the pointer path; Conv1d / Linear load through buffer resources, below),
// ALL issued unconditionally and without a branch (rows past the chunk, taps outside the sequence and channels past the tensor read a
// valid address and are zeroed by the returned mask when they are used -- straight-line code is what lets the compiler count the loads
// in flight: with a branch around a load it waits for vmcnt(0) and the next trip's loads are no longer in flight under this trip's
// products): U rows rbase + S u per lane, 16 bytes of dY and one float of X each.  One 32-bit division per trip (rows < 2^31 and
// n_out >= 8 > S u, so a row is at most ONE utterance further than the trip's first: tu_train.hip wgrad_on_mfma).  Bit u of the
// result: dY valid, bit 8 + u: X valid.
template <int U, int S>
__device__ __forceinline__ unsigned wgrad_issue(const ConvDesc& d, const float* __restrict__ x, const float* __restrict__ dy, long rbase,
                                                long r1, int j, int co4, bool co_ok, int ci, bool ci_ok, f32x4 (&a)[U], float (&bv)[U]) {
    const unsigned rc = (unsigned)(rbase < r1 ? rbase : r1 - 1), n = (unsigned)d.n_out;
    const unsigned b = rc / n, t = rc - b * n;
    const int colA = co_ok ? co4 : 0, colB = ci_ok ? ci : 0;
    unsigned ok = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool rv = rbase + S * u < r1;
        unsigned tu = t + S * u, bu = b;
        const bool wrap = tu >= n;
        tu = rv ? (wrap ? tu - n : tu) : t;
        bu = rv && wrap ? bu + 1 : bu;
        const int q = (int)tu + d.pad - j, qq = q < 0 ? 0 : q;   // ConvTranspose1d: out[n stride + j - pad] += in[n] W[:, :, j]
        int ti = qq / d.stride;
        const bool tv = q >= 0 && ti * d.stride == qq && ti < d.n_in;
        ti = tv ? ti : 0;
        a[u] = ld4(dy + (long)(rv ? rc + (unsigned)(S * u) : rc) * d.c_out + colA);
        bv[u] = x[((long)bu * d.n_in + ti) * d.c_in + colB];
        ok |= ((rv && co_ok) ? 1u : 0u) << u | ((rv && ci_ok && tv) ? 1u : 0u) << (8 + u);
    }
    return ok;
}
template <bool TR>
static __global__ __launch_bounds__(256, 2) void train_conv_wgrad_mfma_kernel(const ConvDesc d, const float* __restrict__ x,
                                                                    const float* __restrict__ dy, float* __restrict__ partial,
                                                                    float* __restrict__ partial_bias, long chunks, long pstride,
                                                                    int chunk_rows, int* __restrict__ dy_absmax = nullptr) {
    // dy_absmax (optional): max |dy| as a by-product -- the (tap 0, first input tile) waves read every element of dY exactly once;
    // an integer atomicMax of the magnitude's bit pattern is order-independent (the data-gradient GEMM that follows derives its
    // power-of-two operand scale from it: no separate pass over dY).
    // The four waves of a workgroup take four consecutive row chunks of the SAME weight tile; their accumulators are added in LDS in
    // wave order (fixed order: reproducible) and ONE partial per workgroup leaves the CU -- the partial sums of the two-stage
    // reduction were this kernel's memory traffic (600 chunks x 64 KB for a decoder convolution at B = 128): four times less now.
    //
    // Round 5: (a) a trip's loads are issued one trip AHEAD of its products (the kernel was a chain of exposed load latencies: ~3 us
    // per 16-row trip whatever the size); (b) chunk_rows follows the problem (tu_train.hip wgrad_chunk: small problems get their
    // parallelism from short chunks); (c) the weight tiles that read the SAME rows of dY are neighbours in one XCD's dispatch order
    // (workgroup n runs on XCD n % 8: with the tile as the fast grid index the four tiles of a decoder convolution sat on four XCDs
    // and each pulled dY through its own L2).  gridDim = (tiles, row groups rounded up to a multiple of 8).
    ESMI_DYN_LDS(red);
    const int lane = lane_id(), i = lane & 31, kh = lane >> 5, w = uniform_i(wave_id());   // (a scalar: the chunk's buffer resource lives in SGPRs)
    const int tci = (d.c_in + 31) / 32;
    const long wg = (long)blockIdx.y * gridDim.x + blockIdx.x, slot = wg >> 3;
    const int tile = (int)(slot % gridDim.x);
    const long ygrp = (slot / gridDim.x) * 8 + (wg & 7);
    if (ygrp * kWgradWaves >= chunks) return;          // (the whole workgroup: in front of every barrier)
    const int j = tile % d.k, ci0 = ((tile / d.k) % tci) * 32, cb = (tile / (d.k * tci)) * 128;
    const long chunk = ygrp * kWgradWaves + w;
    const ChunkRange cr = chunk_range(chunk, chunk_rows, (long)d.B * d.n_out);
    long r0 = cr.r0, r1 = cr.r1;
    const int co4 = cb + 4 * i;                         // this lane's four output channels
    const bool vec_ok = co4 + 3 < d.c_out, ci_ok = ci0 + i < d.c_in;
    f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
    f32x4 bsum = zero4();
    float amax_f = 0.0f;
#if ESMI_CHAIN_SPLIT
    // fp32-accurate split products on the bf16 matrix pipe (esmi_dev.h split_bf16x3: three 8-bit pieces per value = all 24 significand
    // bits, six products, bf16's exponent range -- gradients as small as 1e-30 lose nothing, which binary16 pieces would need a scale
    // for): the contraction runs over the ROWS, so a lane's eight k-slots of a 16-row step are eight consecutive rows -- lane (i, kh)
    // loads dY channels 4i .. 4i+3 and X channel ci0 + i of rows r + 8 kh + (0..7); each of the four dY channels is the A operand of
    // one of four MFMA tiles (channel sets {4m + t}).  24 v_mfma_f32_32x32x16_bf16 (768 cycles) per 16 rows instead of 32
    // v_mfma_f32_32x32x2_f32 (2048 cycles).
    constexpr int kU = 8, kTrip = 16;
#else
    constexpr int kU = 4, kTrip = 8;                   // rows r + 2 u + kh: 8 rows per trip, 16 v_mfma_f32_32x32x2_f32
#endif
    constexpr int kS = kTrip == 16 ? 1 : 2;
    const int lane_row = kTrip == 16 ? 8 * kh : kh;
    const bool stats = j == 0 && ci0 == 0;              // (wave-uniform) the waves that also sum dY's columns and take max |dY|
    if (r0 >= r1) { r0 = 0; r1 = 0; }                   // (chunk >= chunks: no trip; every load below is then out of range and reads 0)
    // one trip's products; `ok` masks what the pointer path (ConvTranspose1d) loaded from a clamped address
    auto products = [&](f32x4 (&a)[kU], float (&bv)[kU], unsigned ok) __attribute__((always_inline)) {
        if (TR) {
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if (!((ok >> u) & 1u)) a[u] = zero4();
                if (!((ok >> (8 + u)) & 1u)) bv[u] = 0.0f;
            }
        }
        if (stats) {
#pragma unroll
            for (int u = 0; u < kU; ++u) {
#pragma unroll
                for (int e = 0; e < 4; ++e) amax_f = fmaxf(amax_f, fabsf(a[u][e]));    // (NaN-transparent enough: a NaN gradient shows up as NaN weights anyway)
                bsum = bsum + a[u];
            }
        }
#if ESMI_CHAIN_SPLIT
        const f32x4 b0 = {bv[0], bv[1], bv[2], bv[3]}, b1 = {bv[4], bv[5], bv[6], bv[7]};
        const bf16x3 b3 = split_bf16x3(b0, b1);
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
            const f32x4 a0 = {a[0][t4], a[1][t4], a[2][t4], a[3][t4]}, a1 = {a[4][t4], a[5][t4], a[6][t4], a[7][t4]};
            acc[t4] = mfma32_split(split_bf16x3(a0, a1), b3.hi, b3.mid, b3.lo, acc[t4]);
        }
#else
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) acc[t4] = mfma32(a[u][t4], bv[u], acc[t4]);
        }
#endif
    };
    // The loads.  Conv1d / Linear: bounds-checked buffer loads, so that nothing is clamped, compared or zeroed per value -- dY through
    // a resource that ends with the chunk's last row (rows past it read 0; a lane's byte offset is its first row's + a wave-uniform
    // multiple of the row size: one add per load), X through a resource over the whole tensor with the offset of (row, tap) kept
    // INCREMENTALLY from trip to trip (n_out >= 16: at most one utterance boundary per trip) and replaced by an out-of-range one where
    // the tap leaves the utterance or the row leaves the chunk.  (Round 5: the loop was VALU-bound on 64-bit address arithmetic, the
    // masks and the register rotation of the look-ahead: 640 VALU instructions, 66 of them quarter rate, per 24 MFMAs.)
    // ConvTranspose1d keeps the pointer path (wgrad_issue).
    constexpr unsigned kBig = 0x7FFFFFFFu;
    const BufRsrc r_dy = make_rsrc(dy + r0 * d.c_out, (r1 - r0) * (long)d.c_out * 4);
    const BufRsrc r_x = make_rsrc(x, (long)d.B * d.n_in * d.c_in * 4);
    const unsigned rowb = (unsigned)d.c_out * 4u, n = (unsigned)d.n_out;
    unsigned dy_off = vec_ok ? (unsigned)(lane_row * d.c_out + co4) * 4u : kBig;        // of this lane's first row of the next trip
    unsigned t_cur, x_off;                                                               // that row's position in its utterance, its X element
    {
        const unsigned rb = (unsigned)(r0 + lane_row), b0 = rb / n;
        t_cur = rb - b0 * n;
        x_off = (unsigned)(((long)b0 * d.n_in + (long)t_cur * d.stride + (j - d.pad)) * d.c_in + ci0 + i) * 4u;   // (mod 2^32 where the tap is outside)
    }
    const unsigned x_step = (unsigned)(d.stride * d.c_in) * 4u, x_wrap = (unsigned)((d.n_in - d.n_out * d.stride) * d.c_in) * 4u;
    long r_next = r0;                                                                    // first row of the next trip to be issued
    auto issue = [&](f32x4 (&a)[kU], float (&bv)[kU]) __attribute__((always_inline)) -> unsigned {
        if (TR) {
            const unsigned ok = wgrad_issue<kU, kS>(d, x, dy, r_next + lane_row, r1 > r0 ? r1 : 1, j, co4, vec_ok, ci0 + i, ci_ok, a, bv);
            const bool any = r_next < r1;
            r_next += kTrip;
            return any ? ok : 0u;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) a[u] = buf_ld4(r_dy, dy_off + (unsigned)(kS * u) * rowb);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const unsigned tu = t_cur + (unsigned)(kS * u);
            const bool wrap = tu >= n;
            const int ti = (int)mul24u(wrap ? tu - n : tu, (unsigned)d.stride) + (j - d.pad);
            const bool okx = ci_ok && (unsigned)ti < (unsigned)d.n_in && r_next + lane_row + kS * u < r1;
            const unsigned off = x_off + (unsigned)(kS * u) * x_step + (wrap ? x_wrap : 0u);
            bv[u] = buf_ld(r_x, okx ? off : kBig);
        }
        {   // this lane's first row of the trip after this one
            t_cur += (unsigned)kTrip;
            const bool wrap = t_cur >= n;
            t_cur = wrap ? t_cur - n : t_cur;
            x_off += (unsigned)kTrip * x_step + (wrap ? x_wrap : 0u);
            dy_off += (unsigned)kTrip * rowb;
            r_next += kTrip;
        }
        return 0x7FFFu;
    };
    // two register sets, each loaded one trip ahead of its products (no rotation: the loop body is two trips)
    f32x4 a0[kU], a1[kU];
    float v0[kU], v1[kU];
    unsigned ok0 = issue(a0, v0), ok1 = 0;
    for (long r = r0; r < r1; r += 2 * kTrip) {
        ok1 = issue(a1, v1);
        sched_fence();
        products(a0, v0, ok0);
        if (r + kTrip >= r1) break;
        ok0 = issue(a0, v0);
        sched_fence();
        products(a1, v1, ok1);
    }
    int amax_i = 0;
    if (dy_absmax && stats) {   // (wave-uniform) this wave's max |dY|; the workgroup's four are combined behind the barrier below
        amax_i = __builtin_bit_cast(int, amax_f) & 0x7FFFFFFF;
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) amax_i = max(amax_i, shfl_i(amax_i, lane ^ dd));
    }
    // ---- sum of the four waves' tiles: wave w0 writes [w0][reg][lane]; wave w then owns accumulator set t4 = w of the sum
    float* mine = red + (w * 64) * 64 + lane;
#pragma unroll
    for (int t4 = 0; t4 < 4; ++t4) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mine[(16 * t4 + r) * 64] = acc[t4][r];
    }
    __syncthreads();
    f32x16 sum = zero16();
#pragma unroll
    for (int w0 = 0; w0 < kWgradWaves; ++w0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sum[r] += red[((w0 * 64) + 16 * w + r) * 64 + lane];
    }
    const long out_row = ygrp * pstride;                 // one partial row per workgroup
    const int ci = ci0 + i;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = cb + 4 * tile_row(r, lane) + w;   // accumulator set t4 = w
        long wi;
        if (co < d.c_out && ci < d.c_in && conv_w_index(d, co, ci, j, &wi)) partial[out_row + wi] = sum[r];
    }
    if (dy_absmax && stats) {
        // ONE atomic per workgroup: 800 device-scope atomics on one address cost a decoder-size launch ~10 us (13 ns each, serialised)
        __syncthreads();
        int* ired = reinterpret_cast<int*>(red);
        if (lane == 0) ired[w] = amax_i;
        __syncthreads();
        if (w == 0 && lane == 0) {
            const int m = max(max(ired[0], ired[1]), max(ired[2], ired[3]));
            if (m > 0) atomicMax(dy_absmax, m);
        }
    }
    if (partial_bias && stats) {                         // bias: column sums of dY, the four waves' again added in wave order
        __syncthreads();
        float* bred = red;                                // [wave][128 channels]
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = bsum[e] + shfl_xor_f(bsum[e], 32);      // even rows (kh = 0) + odd rows (kh = 1)
            if (kh == 0) bred[w * 128 + 4 * i + e] = v;
        }
        __syncthreads();
        if (w == 0 && lane < 64) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int c = lane + 64 * q;
                const float v = ((bred[c] + bred[128 + c]) + bred[256 + c]) + bred[384 + c];
                if (cb + c < d.c_out) partial_bias[out_row + cb + c] = v;
            }
        }
    }
}

}  // namespace esmi
