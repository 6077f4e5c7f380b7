// Fully fused mel decoder -- MelDecoder.forward, layers/networks.py:291-304, plus the length
// regulator gather (networks.py:233-244) on its input side and Phoneme2Mel's final masked_fill
// (networks.py:424-427) on its output side.
//
//   skip = LN(tanh(Linear(d4,dx2)(x)))
//   n_blocks x { x = skip; block_depth x [ x = LN(tanh(Conv1x1(dwConv_k(x)))) ]; skip = LN_s(x + skip) }
//   mel  = Linear(dx2, n_mel)(skip)
//
// One 512-thread workgroup (8 waves) owns a 128-row tile of one utterance; activations live in ONE LDS tile [132][DX2+4] fp32 (two
// zero rows per side = the depthwise conv's in-window padding; +4 floats/row keep the 16-byte row-fragment reads bank-conflict free)
// and never leave the CU.  The first stage (Linear + Tanh + LN) normally runs at PHONEME rate on the encoder side (`h0`); the kernel
// then only gathers.  Two forms of one kernel:
//  * dx2 = 128 (tiny), the WINDOW form: two workgroups per CU, every window its own workgroup with both halos recomputed -- 128 - 2*halo
//    frames are kept, halo = (k/2)*n_blocks*block_depth; LayerNorm by row owners.
//  * dx2 = 256 (small, base), the CHUNK WALK: one workgroup per CU walks a segment of an utterance chunk by chunk; each conv layer's
//    k/2 rows in front of a chunk are carried from the previous chunk, the tile's frame base steps back at every block boundary (BLOCK
//    SKEW: DecWalk, dec_layout.h) so that a chunk advances by 128 - block_depth*k/2 frames, and the LayerNorm runs ON THE K LOOP'S
//    ACCUMULATORS (three barriers per layer instead of four).  Without a workspace it runs the window form.
//
// Weight-stationary GEMMs (ESMI_DEC_SPLIT: exact-fp32 MFMA, or fp32-accurate split products on the f16 matrix pipe).  Wave w = (mh = w>>2, ns = w&3)
// owns rows [64mh, 64mh+64) x columns [ns*DX2/4, +DX2/4).  For each 128-channel K chunk it loads
// its weight slice ONCE into registers (16 coalesced 16-byte loads per 32-column tile, from the
// pre-packed blob) and streams the A fragments of its 64 rows from LDS: the K loop touches no
// global memory.  (Round-1 ablation: with one wave owning 32 full rows, re-streaming the weights
// from L2 for every 32 rows cost 150 us of a 675 us kernel.)
//
// Per conv layer, phases separated by workgroup barriers:
//   1. depthwise k-tap conv IN PLACE on the tile (each thread: 4 channels x 8 or 16 rows, window in registers; the output already split
//      into the K loop's two f16 operand planes);  2. K loop (MFMA only + ds_read_b128), then bias + tanh on the accumulators;
//   3. dx2 = 128: accumulators -> tile, then LayerNorm by row-owner threads (16 threads = one DPP row per tile row, 4 rows per thread so
//      that the gain / shift vectors are read once per 4 rows; the rows' values and the skip tensor in registers; block end:
//      LN_s(x + skip)); dx2 = 256: row statistics through an LDS exchange, accumulators normalised in place and stored once;
//      rows outside [0, L) are forced to 0.
//
// In this file: the phases that are free functions (the row owners' LayerNorm arithmetic, the operand-plane store, the clock stamp),
// then the kernel.  The other phases are `[&]` lambdas or straight-line code inside the kernel: moving them changes the generated
// code of a kernel that sits at its register limit (profiles/dec_refactor_isa.md lists what was tried).
//
// Fidelity notes (SURVEY.md §7 "hard parts"):
//  * frames in [mel_len[b], L) are PADDING FRAMES: zero input rows, but computed like any other frame,
//    because the reference computes them and the k-tap conv leaks them into the last valid frames;
//  * frames outside [0, L) do not exist in the reference: every layer's Conv1d zero-pads there, so
//    such rows are forced to 0 after every LayerNorm;
//  * rows >= mel_len[b] of the output are zeroed only at the very end (the final masked_fill).
#pragma once
#include <type_traits>

#include "dec_layout.h"

// Fixed choices (each the measured best on MI355X; the alternatives and their times are in HISTORY.md 3.1, not in the build):
//  * dx2 = 128: 4 waves per SIMD (128 VGPRs, two workgroups per CU); weight slices of 4 k-steps (split build) / 8 (fp32 build) loaded then
//    used, no hand-pipelined ring (a ring measured 169 -> 172 / 174 us: the neighbour workgroup already fills the L2 round trips);
//  * dx2 = 256 (one workgroup per CU, nobody fills the gaps): the K loop's weight fragments run 2 steps ahead in a VGPR ring
//    (small ES decoder 1774 -> 1687 us; depth 4 spills: 1736), the A fragments one item ahead; 8 waves per window (16: 2.43 vs 1.87 ms).
//  * dx2 = 256: the chunk's mel rows leave as streaming (non-temporal) stores and the h0 row gather runs as streaming loads (base ES,
//    B = 512: HBM traffic per launch 1051 MB with plain stores and loads, 576 MB with streaming mel stores, 541 MB with both, against
//    386 MB algorithmic: profiles/r06_probes/decoder256_traffic_ab.txt);
//  * the utterance's duration scan is copied into LDS (one round trip) and the frame -> phoneme search runs there (a binary search in
//    global memory is log2(T) dependent L2 round trips per chunk: profiles/r06_dec_budget.md); a scan row that does not fit the tile
//    is searched in global memory;
//  * dx2 = 256: LayerNorm on the K loop's accumulators -- per-(row, column slice) sums through a 1 KB-per-32-rows LDS exchange, normalised
//    in registers, stored once (dx2 = 128: tanh rows -> tile -> barrier -> row owners read, normalise, write back).
//  * dx2 = 128, split build: the K loops of the default (three-product) mode run on v_mfma_f32_16x16x32 tiles (4 row tiles x 2 column
//    tiles per wave) instead of v_mfma_f32_32x32x16 (2 x 1): the same wave tile, blob, LDS bytes, weight bytes and matrix-pipe cycles,
//    3 % MORE shader cycles, but on random activations the chip holds a 6 % higher clock under it: tiny decoder 173.1 -> 166.7 us
//    (profiles/r25_decoder_mfma16.md; on zero activations it is 3 % slower).  The one-product modes gain nothing from it (precision 16:
//    118.7 vs 119.0 us; bf16: 144.1 vs 146.4) and keep the 32-row form.  ESMI_DEC_MFMA16 is a mask of the modes that take the 16-row
//    form -- 1 the default mode, 2 precision 16, 4 bf16 -- so every combination builds from this tree (-DESMI_DEC_MFMA16=0 .. 7).
#ifndef ESMI_DEC_MFMA16
#define ESMI_DEC_MFMA16 1
#endif

namespace esmi {

constexpr int kDecWps128 = 4, kDecWeightRing256 = 2;

// max_b mel_len[b], by every wave for itself: one coalesced read, no extra launch, no atomics; the result is made
// wave-uniform (SGPR) at once.
__device__ __forceinline__ int batch_max_len(const int* __restrict__ mel_len, int B) {
    const int lane = lane_id();
    int v = 0;
    for (int j = lane; j < B; j += 64) v = max(v, mel_len[j]);
    float f = row_max32((float)v);      // lengths are far below 2^24: exact in fp32
    f = fmaxf(f, swap32_f(f));
    return uniform_i((int)f);
}

// ================================================================== row-owner LayerNorm: the arithmetic
// LayerNorm of one row of DX2 channels: this thread's NV float4 of it in v[], gain / shift of the same channels in g[] / be[]
// (two-pass; TPR = 16 threads per row, one DPP row: the statistics are 4 DPP adds)
template <int DX2, int NV>
__device__ __forceinline__ void dec_ln_regs(f32x4 (&v)[NV], const f32x4 (&g)[NV], const f32x4 (&be)[NV]) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < NV; ++k) s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
    s = row_sum_n<16>(s);
    const float mean = s * (1.0f / DX2);
    float q = 0.0f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[k][e] -= mean;
            q = fmaf(v[k][e], v[k][e], q);
        }
    }
    q = row_sum_n<16>(q);
    const float rstd = rsqrt_fast_f32(q * (1.0f / DX2) + 1e-5f);   // v_rsq_f32 (1 ulp)
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = fmaf(v[k][e] * rstd, g[k][e], be[k][e]);
    }
}
// a row owner's NV float4 (channel groups c + 16 k) of a parameter vector or of a tile row at `pv`
template <int NV>
__device__ __forceinline__ void dec_owner_ld(const float* pv, f32x4 (&o)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) o[k] = *reinterpret_cast<const f32x4*>(pv + 4 * 16 * k);
}
// four floats -> the two f16 operand planes of a tile row of DX2 channels (row = [DX2 halves h1 | DX2 halves h2 | pad]; esmi_dev.h):
// `base + off` is the dword of the four channels in the first plane
template <int DX2>
__device__ __forceinline__ void dec_store_planes(unsigned* base, int off, const f32x4& v) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    unsigned h1a, h2a, h1b, h2b;
    split_f16_pair(v[0], v[1], h1a, h2a);
    split_f16_pair(v[2], v[3], h1b, h2b);
    unsigned* rowp = base + off;   // (formed here, behind the conversions, where the compiler has always seen it)
    *reinterpret_cast<u32x2*>(rowp) = u32x2{h1a, h1b};
    *reinterpret_cast<u32x2*>(rowp + DX2 / 2) = u32x2{h2a, h2b};
}

// precision 16 (include/esmi.h): four floats -> ONE plane, the nearest binary16 of each (round to nearest even), same dwords as the first
// plane above; the second plane's dwords are neither written nor read
__device__ __forceinline__ void dec_store_plane16(unsigned* base, int off, const f32x4& v) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<u32x2*>(base + off) = u32x2{round_f16_pair(v[0], v[1]), round_f16_pair(v[2], v[3])};   // (checked build: range-noted there)
}

// bf16 (include/esmi.h): the same dwords, the nearest bfloat16 of each (round to nearest even; no range to note)
__device__ __forceinline__ void dec_store_plane_bf16(unsigned* base, int off, const f32x4& v) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<u32x2*>(base + off) = u32x2{round_bf16_pair(v[0], v[1]), round_bf16_pair(v[2], v[3])};
}

// measurement aid (g_dec_clk, dec_layout.h): the FIRST workgroup stamps {shader clock, 100 MHz clock} when it starts -> slot 0, and again
// -> slot 1 at the start of each later chunk (dx2 = 256) / in front of its mel stage (dx2 = 128, one chunk).  (slot 1 - slot 0) is a
// long stretch of the workgroup's life: shader ticks / 100 MHz ticks = the clock the CU ran at.  Both stamps come from ONE workgroup:
// the s_memtime counters of different CUs are not comparable (a first version differenced two workgroups and read 9 GHz on some
// boxes).  No stamp at the very end of the kernel (it costs a spilled register) nor inside the one-chunk kernel's chunk loop (the
// store un-hoists the loop's address arithmetic: 28 spills).
__device__ __forceinline__ void dec_clk_stamp(int ck_) {
    long long* const clk = g_dec_clk;
    if (clk && threadIdx.x == 0) {
        if (blockIdx.x == 0) {
            const int slot = ck_ == 0 ? 0 : 1;
            clk[2 * slot] = clock_shader();
            clk[2 * slot + 1] = clock_real100();
        }
    }
}
template <int MT, int NTW>
__device__ __forceinline__ void dec_zero_acc(f32x16 (&acc)[MT][NTW]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int t = 0; t < NTW; ++t) acc[mt][t] = zero16();
    }
}
template <int RT, int CT>
__device__ __forceinline__ void dec_zero_acc(f32x4 (&acc)[RT][CT]) {   // (the 16-row tiles of ESMI_DEC_MFMA16)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = zero4();
    }
}

// NW waves per window (8 or 16): wave (mh = w>>2, ns = w&3) owns rows [128/MH*mh, +128/MH) x columns [ns*DX2/4, +DX2/4).
// NW = 16 (dx2 = 256, one workgroup per CU either way): four waves per SIMD instead of two inside every barrier-separated
// phase -- the phases are latency-bound, so the extra waves are what hides it -- at 128 VGPRs (one 32-row tile per wave).
// The kernels.  Their body is mel_decoder_body.h, included inside each __global__ definition below (textual inclusion keeps the existing
// kernels' listings what they were; a shared device function did not).  PM is the arithmetic of the contractions (include/esmi.h):
//  DEC_PM_SPLIT  the default: three f16 products per 16-channel step, fp32-accurate (or, in the exact-fp32 build, fp32 MFMAs);
//  DEC_PM_F16    precision 16 (split build only): ONE f16 product per 16-channel step on operands rounded to the nearest binary16 -- the
//                weights' first plane, one activation plane;
//  DEC_PM_BF16   bf16 (split build only): ONE bf16 product per step, nothing scaled -- the activation plane holds nearest-even bfloat16,
//                the weight operand is the nearest-even bfloat16 of (plane 0 + plane 1) * 2^-8, formed in registers from the same blob
//                where the wave loads its slice (bf16_of_f16_planes); the accumulators then hold products with W itself.
// Phases, barriers, LDS layout, grid and the chunk walk are those of the default kernel; every difference is an `if constexpr` on
// P16 / BF / ONE below.
using DecPrecisionMode = PrecisionMode;   // (esmi_types.h; the kernel body's names for its three values:)
constexpr PrecisionMode DEC_PM_SPLIT = PM_SPLIT, DEC_PM_F16 = PM_F16, DEC_PM_BF16 = PM_BF16;
template <int DX2, int KD, int NW, bool HALF16 = false>
__global__ __launch_bounds__(64 * NW, (DX2 <= 128 ? kDecWps128 : NW / 4)) void mel_decoder_kernel(const MelDecP p) {
    constexpr int PM = HALF16 ? DEC_PM_F16 : DEC_PM_SPLIT;
#include "mel_decoder_body.h"
}
// bf16: a __global__ name of its own around the same body
template <int DX2, int KD, int NW>
__global__ __launch_bounds__(64 * NW, (DX2 <= 128 ? kDecWps128 : NW / 4)) void mel_decoder_bf16_kernel(const MelDecP p) {
    constexpr int PM = DEC_PM_BF16;
#include "mel_decoder_body.h"
}

// ---- one instantiation: the launcher and the clock probe's setter of (DX2, KD, PM), declared in dec_layout.h.  Each
// tu_dec_<dx2>_<k>[_p16 | _bf16].hip is ESMI_DEC_INSTANCE(dx2, k, mode) and nothing else: this kernel dominates the library's compile
// time, so the twelve build side by side.  A one-product mode in the exact-fp32 build has no kernel: its unit is then host code alone
// that answers ESMI_ERR_UNSUPPORTED, and tu_decoder.hip's table holds NULL for it.
template <int DX2, int KD, PrecisionMode PM>
int set_dec_clock(long long* slots) { return store_dec_clock_pointer(slots); }

template <int DX2, int KD, PrecisionMode PM>
int launch_mel_decoder(const MelDecP& p, dim3 grid, hipStream_t st) {
    if constexpr (precision_mode_built(PM)) {
        constexpr int NW = 8;   // waves per window (16 for dx2 = 256 measured 30 % slower: HISTORY.md 3.1)
        const int lds = (dec_lds_floats<DX2>(KD) + p.carry_lds_layers * (KD / 2) * DX2) * (int)sizeof(float);
        if constexpr (PM == PM_SPLIT) {
            ESMI_LAUNCH_LDS((mel_decoder_kernel<DX2, KD, NW>), grid, dim3(64 * NW), lds, st, p);
        } else if constexpr (PM == PM_F16) {
            ESMI_LAUNCH_LDS((mel_decoder_kernel<DX2, KD, NW, true>), grid, dim3(64 * NW), lds, st, p);
        } else {
            ESMI_LAUNCH_LDS((mel_decoder_bf16_kernel<DX2, KD, NW>), grid, dim3(64 * NW), lds, st, p);
        }
        return launch_status();
    }
    return ESMI_ERR_UNSUPPORTED;
}

}  // namespace esmi

#define ESMI_DEC_INSTANCE(DX2, KD, PM)                                                                \
    ESMI_TU_RANGE_SETTER(dec_##DX2##_##KD##_##PM)                                                     \
    namespace esmi {                                                                                  \
    template int set_dec_clock<DX2, KD, PM>(long long*);                                              \
    template int launch_mel_decoder<DX2, KD, PM>(const MelDecP&, dim3, hipStream_t);                  \
    }
