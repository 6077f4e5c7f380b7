// What the host side of the mel decoder and its kernel (mel_decoder.h) share: the build knob, the window constants, the packed blob
// (its packing kernels and its layout), the kernel's argument block, the LDS sizing, the chunk walk's arithmetic, the clock probe and
// the table of instantiations.  tu_decoder.hip (packer, launcher) needs nothing else of the decoder.
#pragma once
#include "esmi_dev.h"
#include "small_kernels.h"

// Build knob: the contraction form (two libraries of one ABI are built from it, __graft_entry__.py)
#ifndef ESMI_DEC_SPLIT      // contraction of the pointwise GEMMs (esmi_dev.h):
#define ESMI_DEC_SPLIT 2    //   0: v_mfma_f32_32x32x2_f32 (exact fp32; the libesmi_fp32mfma.so build)
#endif                      //   2: fp32 split into 2 f16 (weights pre-scaled by 2^8), 3 products on v_mfma_f32_32x32x16_f16
#if ESMI_DEC_SPLIT != 0 && ESMI_DEC_SPLIT != 2
#error "ESMI_DEC_SPLIT must be 0 (fp32 MFMA) or 2 (split f16x2)"
#endif
#if (ESMI_DEC_SPLIT == 2) != (ESMI_CHAIN_SPLIT != 0)   // one build, one answer to "are the one-product paths there?" (launch.h precision_mode_built)
#error "ESMI_DEC_SPLIT and ESMI_CHAIN_SPLIT go together: both split (2, 1) or both exact fp32 (0, 0)"
#endif

namespace esmi {

constexpr int kDecRows = 128;     // frames per workgroup window
constexpr int kDecPadRows = 2;    // zero rows above/below the window in LDS (>= k/2)
constexpr int kDecThreads = 512;  // 8-wave windows (the dx2 = 128 kernel and the host-side launch default)
constexpr int kMelCols = 96;      // n_mel <= 96 (three 32-column MFMA tiles)

// Weight-stationary B-fragment packing of a (N, K) row-major matrix, K a multiple of 128, for a
// workgroup whose 4 column slices are WCOLS = 32*NTW wide:
//   dst[(((((c*4 + ns)*NTW + ntw)*16 + kc)*64 + lane)*4 + s] =
//       W[ns*WCOLS + 32*ntw + (lane&31)][128*c + 8*kc + 4*(lane>>5) + s]      (0 for rows >= N)
static __global__ void pack_bslice_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int K, int NTW) {
    const long n = (long)(K / 128) * 4 * NTW * 16 * 256;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int s = (int)(e & 3);
        const int lane = (int)((e >> 2) & 63);
        long q = e >> 8;
        const int kc = (int)(q & 15); q >>= 4;
        const int ntw = (int)(q % NTW); q /= NTW;
        const int ns = (int)(q & 3);
        const int c = (int)(q >> 2);
        const int row = ns * 32 * NTW + 32 * ntw + (lane & 31);
        const int col = 128 * c + 8 * kc + 4 * (lane >> 5) + s;
        dst[e] = row < N ? src[(long)row * K + col] : 0.0f;
    }
}

// The same slices as two binary16 planes of 2^8 * W (round to nearest; esmi_dev.h) in the B layout of v_mfma_f32_32x32x16_f16:
// per (chunk c, column slice ns, tile ntw, 16-channel step s, plane p) 64 lanes x 4 dwords,
//   row = ns*32*NTW + 32*ntw + (lane&31),  k0 = 128*c + 16*s + 8*(lane>>5) + 2*w       (0 for rows >= N)
//   dst[((((((c*4 + ns)*NTW + ntw)*8 + s)*2 + p)*64 + lane)*4 + w] = {plane_p(W[row][k0 + 1]), plane_p(W[row][k0])}
static __global__ void pack_bslice2h_kernel(const float* __restrict__ src, unsigned* __restrict__ dst, int N, int K, int NTW) {
    const long n = (long)(K / 128) * 4 * NTW * 8 * 2 * 256;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const int wd = (int)(e & 3);
        const int lane = (int)((e >> 2) & 63);
        long q = e >> 8;
        const int pl = (int)(q & 1); q >>= 1;
        const int st = (int)(q & 7); q >>= 3;
        const int ntw = (int)(q % NTW); q /= NTW;
        const int ns = (int)(q & 3);
        const int c = (int)(q >> 2);
        const int row = ns * 32 * NTW + 32 * ntw + (lane & 31);
        const int k0 = 128 * c + 16 * st + 8 * (lane >> 5) + 2 * wd;
        unsigned half[2];
        for (int j = 0; j < 2; ++j) {
            const float x = (row < N ? src[(long)row * K + k0 + j] : 0.0f) * kF16WScale;
            const unsigned h1 = f32_to_f16_bits(x, false);
            half[j] = pl == 0 ? h1 : f32_to_f16_bits(x - f16_bits_to_f32(h1), false);
        }
        dst[e] = half[0] | (half[1] << 16);
    }
}

// The blob's layout, offsets in floats -- the one description the packer writes by and the kernel reads by:
//   proj matrix | proj_b, proj_g, proj_beta | per conv layer: taps[kd][dx2], dw_b, pw_b, ln_g, ln_b, then the packed pointwise matrix |
//   per block: skip gain[dx2], bias[dx2] | mel matrix (packed like a dx2 x dx2 matrix, rows >= n_mel zero) | mel_b (zero padded to dx2)
// A matrix takes DX2 * DX2 floats either way: two f16 planes or fp32 are the same bytes.
// Everything inside a conv layer is a compile-time offset (DX2, KD are template parameters), and the few run-time offsets are 32-bit (the
// blob is a few MB; the host refuses one that they would not hold, see `floats`).  The kernel used
// to take the 16 64-bit fields of a run-time layout as arguments: 32 SGPRs live across the layer loop, which is where the dx2 = 256
// kernel's SGPR spills (48) and its uniform values in VGPRs came from.
template <int DX2, int KD>
struct DecLay {
    static constexpr int proj_w = 0, l_dw = 0, l_dwb = KD * DX2, l_pwb = l_dwb + DX2, l_g = l_pwb + DX2, l_b = l_g + DX2, l_pw = l_b + DX2,
                         layer_stride = l_pw + DX2 * DX2;
    int proj_b, layer0, skip0, mel_w, mel_b, total;
    __host__ __device__ DecLay(int d4, int n_blocks, int block_depth) {
        proj_b = d4 * DX2;                     // proj_b, proj_g, proj_beta contiguous
        layer0 = proj_b + 3 * DX2;
        skip0 = layer0 + layer_stride * n_blocks * block_depth;
        mel_w = skip0 + 2 * DX2 * n_blocks;
        mel_b = mel_w + DX2 * DX2;
        total = mel_b + DX2;
    }
    // `total` in 64 bits, for the host: the blob's size, and the test against kDecBlobMaxFloats before anything trusts the 32-bit fields
    static long floats(int d4, int n_blocks, int block_depth) {
        return ((long)d4 + 3) * DX2 + (long)layer_stride * n_blocks * block_depth + 2L * DX2 * n_blocks + ((long)DX2 + 1) * DX2;
    }
};
constexpr long kDecBlobMaxFloats = 0x1fffffffL;   // what the offsets above and the kernel's 32-bit byte offsets hold

struct MelDecP {
    const float* blob;
    int d4, n_blocks, block_depth, n_mel;
    const float* x;        // (B,T,d4) phoneme-rate (cum != NULL) or (B,L,d4) frame-rate
    const float* h0;       // optional (cum != NULL): (B,T,dx2) = LN(tanh(proj(x))) already computed at PHONEME rate
    const int* cum;        // (B,T) inclusive duration cumsum or NULL
    const int* mel_len;    // (B) or NULL
    const int* lmax_dev;   // device scalar or NULL
    int lmax_host;
    int apply_mask;
    int B, T, L_out;
    float* mel;            // (B, L_out, n_mel)
    int halo;              // rows a window loses per side without carried state: (k/2) * conv layers
    int seg_len;           // frames per segment (a workgroup's share of an utterance)
    int n_seg;             // segments per utterance
    float* carry_ws;       // dx2 = 256 with multi-chunk segments: per workgroup `ws_stride` floats of scratch ([conv layer slot][k/2][dx2],
                           // then [block boundary][kDecBlockCarry4 float4]), else NULL
    int ws_stride;
    int carry_lds_layers;  // conv-layer carry slots kept in LDS behind the tile (what fits); the rest live in `carry_ws`
    int skew;              // dx2 = 256 chunk walk: the tile's frame base steps back by block_depth * k/2 rows at every block boundary
                           // (a chunk then loses block_depth * k/2 rows on its right instead of the whole halo), see DecWalk
    long long* trace;      // development only (-DESMI_DEC_TRACE): [wave][stamp] shader-clock stamps of block (1,0)
};
// measurement aid (esmi_mel_decoder_clock_probe, include/esmi.h): two {shader clock, 100 MHz clock} stamps per launch, see the chunk
// loop.  A device global per translation unit (like the range flag), not a kernel argument: the kernel is at its register limit.
ESMI_DEVICE_GLOBAL_PTR(long long, g_dec_clk);
static inline int store_dec_clock_pointer(long long* slots) { return ESMI_STORE_DEVICE_GLOBAL_PTR(g_dec_clk, slots); }

// block skew: a block boundary hands (block_depth + 1) * k/2 rows of dx2 floats to the next chunk, one float4 per thread
constexpr int kDecBlockCarry4 = 512;
// LDS floats of a workgroup: the tile, the parameter slots, the frame sources and (dx2 = 256) the LayerNorm statistics exchange
template <int DX2>
__host__ __device__ constexpr int dec_lds_floats(int kd) {
    return (kDecRows + 2 * kDecPadRows) * (DX2 + 4) + (kd + 6) * DX2 + kDecRows + (DX2 > 128 ? 2 * kDecRows * 8 : 0);
}
// conv layers whose carried rows (k/2 rows of dx2 floats each) fit in LDS behind the tile and the parameter slots (dx2 = 256 only)
template <int DX2>
inline int dec_carry_lds_layers(int kd, int n_layers) {
    if (DX2 <= 128) return 0;
    const int free_f = 160 * 1024 / 4 - dec_lds_floats<DX2>(kd), per = (kd / 2) * DX2;
    const int n = free_f / per;
    return n < n_layers ? n : n_layers;
}

// THE CHUNK WALK (dx2 = 256 with a workspace; the kernel's chunk loop has the story).  A workgroup walks its segment of an utterance in
// chunks of one 128-row tile.  Without the block skew every chunk loses `halo` rows on its right and advances by 128 - halo frames.
// BLOCK SKEW (round 6): inside a block the tile's rows keep their frames, so every conv layer costs k/2 valid rows on the right: `sh` =
// block_depth * k/2 per block; at a block boundary the rows move `sh` rows down and the top `sh` rows come from the previous chunk, so
// the next block starts with 128 valid rows again, `sh` frames earlier.  A chunk therefore advances by keep = 128 - sh frames (base ES
// 122, small 124) instead of 128 - halo (110 / 116); tile row r of block b holds frame g0 + (n_blocks - 1 - b) * sh + r.
// Used when the model has more than one block and a block carry fits one float4 per thread:
__host__ __device__ inline bool dec_walk_skew(int dx2, int kd, int n_blocks, int block_depth) {
    return n_blocks >= 2 && (block_depth + 1) * (kd / 2) * (dx2 / 4) <= kDecBlockCarry4;
}
struct DecWalk {
    bool skew;
    int halo, n_blocks;
    int sh;     // rows the tile's frame base steps back at a block boundary (0 without the skew)
    __host__ __device__ DecWalk(bool skew_, int pad, int n_blocks_, int block_depth, int halo_)
        : skew(skew_), halo(halo_), n_blocks(n_blocks_), sh(skew_ ? pad * block_depth : 0) {}
    // frames in front of an utterance's first output frame: the last block's tile starts that much early
    __host__ __device__ int lead() const { return sh * (n_blocks - 1); }
    // rows a segment that starts inside an utterance recomputes (nothing is carried into its first chunk)
    __host__ __device__ int lost() const { return skew ? 2 * halo - sh : halo; }
    // tile rows of a chunk that stay valid through every layer = frames a chunk advances by
    __host__ __device__ int keep() const { return skew ? kDecRows - sh : kDecRows - halo; }
};

// One translation unit per instantiation (tu_dec_<dx2>_<k>[_p16 | _bf16].hip: the kernel is by far the slowest thing to compile) defines
// these two for its (DX2, KD, PM) by explicit instantiation -- ESMI_DEC_INSTANCE, mel_decoder.h, where the definitions are.  Declarations
// only here: tu_decoder.hip takes their addresses for its table of instantiations and must not see the definitions (it includes this
// header, never mel_decoder.h), or it would instantiate the kernels itself.
template <int DX2, int KD, PrecisionMode PM>
int launch_mel_decoder(const MelDecP& p, dim3 grid, hipStream_t st);
template <int DX2, int KD, PrecisionMode PM>
int set_dec_clock(long long* slots);

}  // namespace esmi
