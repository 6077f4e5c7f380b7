// reg_tile -- device toolkit of the register-resident encoder kernels (enc_va64.h, enc_ffn64.h, enc_pred128.h, enc_fuse128.h,
// enc_ffn128.h, enc_merge256.h): activations stay in registers from GEMM to GEMM, LDS holds the weights and the rows across tile
// boundaries.
//
// Layout (chain16.h): a wave owns 16-row tiles, products are transposed -- lane (i, g) holds row i and, per 16-channel output tile nt,
// channels 16 nt + 4 g + (0..3).  A row of KG k groups (32 KG channels) is the operand f16x2p[KG] of the next GEMM.
//   * to_bop: a GEMM's output becomes the next GEMM's second operand IN REGISTERS: that operand wants channels {c0..c0+3, c0+8..c0+11},
//     c0 = 32 G + 16 (g >> 1) + 4 (g & 1), of the lane's row -- the lane's own four channels of tile 2 G (g < 2) or 2 G + 1 (g >= 2)
//     plus its partner's (lane ^ 32): one v_permlane32_swap per register, then the f16 split;
//   * rows_dn / rows_up: the row -+ 1 operands of a k = 3 tap by DPP row shifts inside the 16 lanes that hold a tile's rows for one g;
//     the lane at the tile's edge takes the neighbouring tile's row from the boundary-row exchange buffer in LDS (bnd_*), [tile][side]
//     [k group KG][piece 2][16 dwords];
//   * a weight set = a packed matrix of NT / 2 row tiles of 32 (esmi_pack_bfrag_f32) in LDS; kgroup multiplies one k group of it with
//     the operands of one or more tiles, four 16-channel output tiles at a time, every fragment read once for all tiles;
//   * the weight sets stream through two LDS buffers filled by LDS-DMA one step ahead, one workgroup barrier per step (step_begin).
#pragma once
#include "chain16.h"

namespace esmi {

constexpr int kRegTileMaxWaves = 8;   // one workgroup per utterance: eight waves x two 16-row tiles = 256 rows

namespace rt {
using namespace c16;

// rows one down / one up inside the 16 lanes that hold a tile's rows for one g (row_dn_u / row_up_u, wavesim_shim.h): the lane at the
// tile's edge takes `edge` (the neighbouring tile's row, or zero outside the sequence)
__device__ __forceinline__ f16x2p rows_dn(const f16x2p& x, const f16x2p& edge) {
    f16x2p o;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o.h1[e] = row_dn_u(x.h1[e], edge.h1[e]); o.h2[e] = row_dn_u(x.h2[e], edge.h2[e]); }
    return o;
}
__device__ __forceinline__ f16x2p rows_up(const f16x2p& x, const f16x2p& edge) {
    f16x2p o;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o.h1[e] = row_up_u(x.h1[e], edge.h1[e]); o.h2[e] = row_up_u(x.h2[e], edge.h2[e]); }
    return o;
}
__device__ __forceinline__ f16x2p zero_bop() {
    f16x2p o;
    o.h1 = u32x4{0u, 0u, 0u, 0u};
    o.h2 = u32x4{0u, 0u, 0u, 0u};
    return o;
}
// D^T rows (2 KG tiles of 16 channels) -> the second operand of the next GEMM's KG k groups (see the header)
template <int KG>
__device__ __forceinline__ void to_bop(const f32x4 (&v)[2 * KG], f16x2p (&out)[KG], bool lower) {
#pragma unroll
    for (int G = 0; G < KG; ++G) {
        f32x4 recv;
#pragma unroll
        for (int e = 0; e < 4; ++e) recv[e] = swap32_f(lower ? v[2 * G + 1][e] : v[2 * G][e]);
        out[G] = split_f16x2(lower ? v[2 * G] : recv, lower ? recv : v[2 * G + 1]);
    }
}

// ---- boundary rows: dword index of (tile, side, k group, piece) for lane group g
template <int KG>
__device__ __forceinline__ int bnd_at(int tile, int side, int G, int piece, int g) { return ((tile * 2 + side) * (2 * KG) + G * 2 + piece) * 16 + 4 * g; }
// the lane's row X as (tile, side)
template <int KG>
__device__ __forceinline__ void bnd_store(unsigned* bnd, int tile, int side, int g, const f16x2p (&X)[KG]) {
#pragma unroll
    for (int G = 0; G < KG; ++G) {
        *reinterpret_cast<u32x4*>(bnd + bnd_at<KG>(tile, side, G, 0, g)) = X[G].h1;
        *reinterpret_cast<u32x4*>(bnd + bnd_at<KG>(tile, side, G, 1, g)) = X[G].h2;
    }
}
// the first (side 0) and last (side 1) rows of the wave's tiles tile0 ..
template <int NTILE, int KG>
__device__ __forceinline__ void bnd_publish(unsigned* bnd, int tile0, int i, int g, const f16x2p (&X)[NTILE][KG]) {
#pragma unroll
    for (int t = 0; t < NTILE; ++t) {
        if (i == 0 || i == 15) bnd_store<KG>(bnd, tile0 + t, i == 0 ? 0 : 1, g, X[t]);
    }
}
template <int KG>
__device__ __forceinline__ f16x2p bnd_read(const unsigned* bnd, int tile, int side, int G, int g, bool exists) {
    f16x2p o = zero_bop();
    if (exists) {
        o.h1 = *reinterpret_cast<const u32x4*>(bnd + bnd_at<KG>(tile, side, G, 0, g));
        o.h2 = *reinterpret_cast<const u32x4*>(bnd + bnd_at<KG>(tile, side, G, 1, g));
    }
    return o;
}

// ---- GEMMs against one weight set in LDS (NT = 2 x its 32-row tiles; lw = wlane(lane, NT / 2))
// acc[t][nt] += W[16 nt + .., 32 G + ..] . op[t]^T for every tile t: one k group, four output tiles at a time (their fragments are 32
// registers), every fragment read once for all NTILE tiles
template <int NTILE, int NT>
__device__ __forceinline__ void kgroup(f32x4 (&acc)[NTILE][NT], const float* W, int lw, int G, const f16x2p (&op)[NTILE]) {
#pragma unroll
    for (int ch = 0; ch < NT / 4; ++ch) {
        WFrags<4> wf;
        wfrags_load<4, NT / 2, 4>(wf, 0, W + 2 * ch * 256, lw, G);
#pragma unroll
        for (int t = 0; t < NTILE; ++t) mma_all<4>(*reinterpret_cast<f32x4 (*)[4]>(&acc[t][4 * ch]), wf, op[t]);
    }
}
template <int NT>
__device__ __forceinline__ void kgroup(f32x4 (&acc)[NT], const float* W, int lw, int G, const f16x2p& op) {
    kgroup(*reinterpret_cast<f32x4 (*)[1][NT]>(&acc), W, lw, G, *reinterpret_cast<const f16x2p (*)[1]>(&op));
}
// acc[t] += W[.., 32 (G0 + G) ..] . X[t][G]^T for G < KS
template <int NTILE, int NT, int KS>
__device__ __forceinline__ void set_gemm(f32x4 (&acc)[NTILE][NT], const float* W, int lw, const f16x2p (&X)[NTILE][KS], int G0 = 0) {
#pragma unroll
    for (int G = 0; G < KS; ++G) {
        f16x2p op[NTILE];
#pragma unroll
        for (int t = 0; t < NTILE; ++t) op[t] = X[t][G];
        kgroup(acc, W, lw, G0 + G, op);
    }
}
template <int NT, int KS>
__device__ __forceinline__ void set_gemm(f32x4 (&acc)[NT], const float* W, int lw, const f16x2p (&X)[KS], int G0 = 0) {
#pragma unroll
    for (int G = 0; G < KS; ++G) kgroup(acc, W, lw, G0 + G, X[G]);
}
// tap j of a k = 3 convolution: c[t][nt] += W_j . X^T(row + j - 1) over the KG k groups, for the tiles tile0 + t of ntiles; W = the
// tap's weight set, bnd = the boundary rows of X
template <int NTILE, int NT, int KG>
__device__ __forceinline__ void conv_tap(f32x4 (&c)[NTILE][NT], const float* W, int lw, int j, const f16x2p (&X)[NTILE][KG], const unsigned* bnd,
                                         int tile0, int ntiles, int g) {
#pragma unroll
    for (int G = 0; G < KG; ++G) {
        f16x2p op[NTILE];
#pragma unroll
        for (int t = 0; t < NTILE; ++t) {
            const int tile = tile0 + t;
            if (j == 0) op[t] = rows_dn(X[t][G], bnd_read<KG>(bnd, tile - 1, 1, G, g, tile > 0));
            else if (j == 1) op[t] = X[t][G];
            else op[t] = rows_up(X[t][G], bnd_read<KG>(bnd, tile + 1, 0, G, g, tile + 1 < ntiles));
        }
        kgroup(c, W, lw, G, op);
    }
}
template <int NT, int KG>
__device__ __forceinline__ void conv_tap(f32x4 (&c)[NT], const float* W, int lw, int j, const f16x2p (&X)[KG], const unsigned* bnd, int tile,
                                         int ntiles, int g) {
    conv_tap(*reinterpret_cast<f32x4 (*)[1][NT]>(&c), W, lw, j, *reinterpret_cast<const f16x2p (*)[1][KG]>(&X), bnd, tile, ntiles, g);
}

// ---- the two-buffer weight pipeline
// step k begins: this wave's share of set k has landed, every wave is through step k - 1 (the other buffer is free, what step k - 1
// wrote to LDS is visible); then set k + 1 is requested into the buffer step k - 1 used.  request(k) = the kernel's own schedule.
template <typename Request>
__device__ __forceinline__ void step_begin(int k, int nset, Request& request) {
    wait_vm0();
    wg_sync_lds();
    if (k >= 1 && k + 1 < nset) request(k + 1);
}
// dma_frags for a 128-row weight set cut out of a packed array with `ntw` row tiles per (k group, slot): fragment fr (k group, slot,
// row tile) <- src[((fr >> 2) ntw + (fr & 3)) 256]
__device__ __forceinline__ void dma_cut(const float* src, int ntw, float* dst, int w, int nw, int lane, int rot) {
    for (int f = w; f < 64; f += nw) {
        const int fr = (f + rot) & 63;
        lds_dma16(src + ((fr >> 2) * ntw + (fr & 3)) * 256 + 4 * lane, dst + fr * 256, lane);
    }
}

}  // namespace rt
}  // namespace esmi
