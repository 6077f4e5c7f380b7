// Host-side glue shared by the translation units of libesmi.so: stream / status helpers and the internal launchers
// (one per kernel family; each is defined in the one translation unit that instantiates that family's kernels, so the
// families compile in parallel and a kernel edit rebuilds one file).  Not part of the C-ABI (include/esmi.h is).
#ifndef ESMI_LAUNCH_H
#define ESMI_LAUNCH_H
#include "../../include/esmi.h"

#include <cmath>
#include <cstring>

#include "attention.h"
#include "convgemm.h"
#include "pwgemm.h"
#include "hifigan_resblock.h"
#include "enc_attn_ffn.h"
#include "enc_fuse_va.h"
#include "enc_merge_qkv.h"
#include "enc_params.h"
#include "esmi_dev.h"
#include "small_kernels.h"

namespace esmi {

inline hipStream_t S(esmi_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ESMI_OK : (int)e;
}
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The `precision` of the C entry points and of esmi_conv_desc (include/esmi.h: 0 / 32, 16, ESMI_PRECISION_BF16) as the mode every
// launcher below speaks (PrecisionMode, esmi_types.h); ESMI_ERR_ARG for anything else.
inline int precision_mode(int precision, PrecisionMode* mode) {
    switch (precision) {
        case 0:
        case 32: *mode = PM_SPLIT; return ESMI_OK;
        case 16: *mode = PM_F16; return ESMI_OK;
        case ESMI_PRECISION_BF16: *mode = PM_BF16; return ESMI_OK;
    }
    return ESMI_ERR_ARG;
}
// Does this build have the mode's kernels?  The exact-fp32 library (ESMI_CHAIN_SPLIT = 0 and ESMI_DEC_SPLIT = 0, one knob in two
// spellings: dec_layout.h) has no one-product path; an entry point answers ESMI_ERR_UNSUPPORTED there.
constexpr bool precision_mode_built(PrecisionMode mode) { return mode == PM_SPLIT || ESMI_CHAIN_SPLIT; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE setting: remember per (instantiation, device ordinal) that
// it was made (once: keeps the call out of hipGraph captures).  `done` is one static table per call site.
constexpr int kMaxDevices = 64;
struct AttrOnce { bool done[kMaxDevices] = {}; };
inline int raise_lds_limit(const void* fn, AttrOnce& once) {
    const int dev = current_device();
    if (dev < 0) return -dev;
    if (dev >= kMaxDevices) return ESMI_ERR_UNSUPPORTED;
    if (!once.done[dev]) {
        if (int rc = set_max_dynamic_lds(fn, 160 * 1024)) return rc;
        once.done[dev] = true;
    }
    return ESMI_OK;
}
// raise_lds_limit once per call site, then ESMI_LAUNCH; returns the error from the enclosing launcher.  (A macro: ESMI_LAUNCH
// stringifies the kernel for the simulator's launch log.)
#define ESMI_LAUNCH_LDS(kern, grid, block, lds, stream, ...)                                                                   \
    do {                                                                                                                       \
        static AttrOnce once_;                                                                                                 \
        if (int rc_ = raise_lds_limit(reinterpret_cast<const void*>(kern), once_)) return rc_;                                 \
        ESMI_LAUNCH(kern, grid, block, lds, stream, __VA_ARGS__);                                                              \
    } while (0)
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int conv_out_len(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }
inline unsigned grid1d(long n, int block = 256) { return (unsigned)((n + block - 1) / block); }

// tu_convgemm.hip
ConvGemmP conv_defaults();
int launch_convgemm(ConvGemmP p, hipStream_t st);
int launch_conv_to1_len(ConvGemmP p, int16_t* pcm, hipStream_t st);   // ConvGemmP::len set: zeros behind each utterance's end; float and / or int16 plane
// The ops of the one-kernel-per-op plan as ConvGemmP descriptors: the shape and operand fields, filled in one place.  What tells one op
// from the next (activation, residual, LayerNorm, masks, row-dot, accumulation, column offsets, ...) stays an assignment at the call site.
struct ConvW { const float *w, *wp; };   // the fp32 tensor (k, c_out, c_in) and its pre-split blob (esmi_pack_bfrag_f32); either may be NULL
inline ConvGemmP linear(int B, int n, int c_in, int c_out, const float* A, int lda, ConvW w, const float* bias, float* out, int ldo) {
    ConvGemmP p = conv_defaults();
    p.B = B; p.n_in = p.n_out = n; p.c_in = c_in; p.c_out = c_out;
    p.A = A; p.lda = lda; p.W = w.w; p.Wp = w.wp; p.bias = bias; p.out = out; p.ldo = ldo;
    return p;
}
// Conv1d(c_in, c_out, k, dilation = dil, padding = "same"), stride 1.  (dil = 1 is stored as 1; the kernels read 0, conv_defaults', as 1 too)
inline ConvGemmP conv1d(int B, int n, int c_in, int c_out, int k, int dil, const float* A, int lda, ConvW w, const float* bias, float* out, int ldo) {
    ConvGemmP p = linear(B, n, c_in, c_out, A, lda, w, bias, out, ldo);
    p.k = k; p.dil = dil; p.pad = (k * dil - dil) / 2;
    return p;
}
// ConvTranspose1d(c_in, c_out, k, stride, padding = pad): n_in -> n_out positions (n_out below the full length crops)
inline ConvGemmP conv_transpose1d(int B, int n_in, int n_out, int c_in, int c_out, int k, int stride, int pad, const float* A, int lda,
                                  ConvW w, const float* bias, float* out, int ldo) {
    ConvGemmP p = linear(B, n_in, c_in, c_out, A, lda, w, bias, out, ldo);
    p.n_out = n_out; p.mode = MODE_CONVT; p.k = k; p.stride = stride; p.pad = pad;
    return p;
}
// tu_convgemm_bf16.hip: the three GEMM families with bfloat16 operands (ConvGemmP::amp == 2, the training step's bf16-mixed precision).
// launch_convgemm decides the family, the tiling and the grid exactly as for the other precisions and hands them over
int launch_convgemm_stream_bf16(const ConvGemmP& p, int nt, dim3 grid, hipStream_t st);
// the length-limited streaming kernel (ConvGemmP::len) with bfloat16 operands: the generator's limited stages at bf16
int launch_convgemm_len_bf16(const ConvGemmP& p, int nt, dim3 grid, hipStream_t st);
#if ESMI_CHAIN_SPLIT
int launch_pwgemm_bf16(const ConvGemmP& p, bool full_row, dim3 grid, int n_items, hipStream_t st);
int launch_convgemm_dma_bf16(const ConvGemmP& p, bool wide, int mt, dim3 grid, int lds_bytes, int nx, int ny, hipStream_t st);
#endif
// tu_attention.hip
int launch_attn(const AttnP& p, hipStream_t st);
// tu_enc_merge.hip / tu_enc_block.hip / tu_enc_attn_ffn.hip / tu_enc_fuse_va.hip (rounds 1-4: the 32-row wave-chain kernels).  Every
// launcher answers ESMI_ERR_UNSUPPORTED for a shape it is not built for; which plan bits apply is decided by its caller (esmi_abi.hip).
int launch_enc_merge_qkv(const EncMergeP& p, int c_in, int c_out, hipStream_t st);
int launch_enc_block(const EncAttnFfnP& p, int expansion, int c_in, bool split2, hipStream_t st);   // split2: two waves per row tile
int launch_enc_attn_ffn(const EncAttnFfnP& p, int expansion, bool split2, hipStream_t st);
int launch_enc_fuse_va(const FuseVaP& p, int dim, int kernel, int nw, bool head, hipStream_t st);
// tu_enc_block16.hip / tu_enc_va16.hip (round 5: dim = 32 models on 16-row tiles, weights through LDS)
int launch_enc_block16(const EncAttnFfnP& p, int expansion, int c_in, hipStream_t st);
int launch_enc_va16(const FuseVaP& p, int dim, int kernel, hipStream_t st);
bool enc_va16_ok(const FuseVaP& p, int dim, int kernel);
// ... and the whole encoder side in one launch (block 0 | block 1 | Fuse + variance adaptor), when each of the three chain16 kernels
// serves its shape and they run the same number of waves
int launch_enc_all16(const EncAttnFfnP& b0, const EncAttnFfnP& b1, int c_in1, const FuseVaP& va, int dim, int kernel, hipStream_t st);
// tu_enc_va64.hip / tu_enc_pred128.hip (round 6: activations in registers, weights streamed through LDS; one workgroup per utterance)
int launch_enc_va64(const FuseVaP& p, int dim, int kernel, hipStream_t st);   // enc_va64.h: Fuse + variance adaptor of a dim = 64 model, T <= 256
int launch_enc_post_attn64(const PostAttn64P& p, hipStream_t st);   // enc_ffn64.h: proj + LN1 + MixFFN + LN2 of a C = 64 one-head block, N <= 256
int launch_enc_pred128(const Pred128P& p, int dim, hipStream_t st);   // enc_pred128.h: three predictors + tail + scan, dim = 128, T <= 256
int launch_enc_fuse128(const FuseVaP& p, int dim, int kernel, hipStream_t st);   // enc_fuse128.h: the Fuse stage of the same models
int launch_enc_post_attn128(const PostAttn128P& p, hipStream_t st);   // enc_ffn128.h: proj + LN1 + MixFFN + LN2, C = 128, two heads, expansion 2, N <= 256
int launch_enc_merge_q256(const MergeQ256P& p, hipStream_t st);   // enc_merge256.h: merge conv k = 3 stride 2, 128 -> 256, + the folded query GEMM, N <= 128

// ---- One HiFi-GAN ResBlock in one launch (hifigan_resblock.h) when its packed weights are there and (channels, kernel size) has an
// instantiation; the generator's resblock_fused_ok (tu_hifigan.hip) decides and sizes the window, else the block runs conv by conv.
// The (c, k) ladder, once for the three modes.  What the one-product kernels do differently: one operand plane in LDS instead of two
// (rb_amp_lds_bytes), 16 waves at 64 channels (rb_amp_waves), and a window of at most rb_amp_rmax(c) rows.
template <PrecisionMode PM, int C, int K>
int launch_resblock_ck(const ResblockP& p, hipStream_t st) {
    constexpr bool kOne = PM != PM_SPLIT;
    const size_t lds = kOne ? rb_amp_lds_bytes(C, p.R) : rb_lds_bytes(C, p.R);
    const dim3 grid((unsigned)(p.B * p.tiles_per_b)), block(64 * (kOne ? rb_amp_waves(C) : kRbWaves));
    if (kOne && p.R > rb_amp_rmax(C)) return ESMI_ERR_ARG;   // (rows past the waves' items would never be computed)
    if constexpr (C <= 16) {   // narrow MFMA tiles (16 channels x 16 positions): LDS <= 32 KB, no limit to raise
        if constexpr (PM == PM_SPLIT) {
            ESMI_LAUNCH((hifigan_resblock16_kernel<C, K>), grid, block, lds, st, p);
        } else if constexpr (PM == PM_F16) {
            ESMI_LAUNCH((hifigan_resblock16_amp_kernel<C, K>), grid, block, lds, st, p);
        } else {
            ESMI_LAUNCH((hifigan_resblock16_bf16_kernel<C, K>), grid, block, lds, st, p);
        }
    } else {
        static AttrOnce once;
#define ESMI_RB_LAUNCH(kern)                                                                                       \
    do {                                                                                                           \
        if (lds > 48 * 1024)                                                                                       \
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(kern), once)) return rc;                    \
        ESMI_LAUNCH(kern, grid, block, lds, st, p);                                                                \
    } while (0)
        if constexpr (PM == PM_SPLIT) {
            ESMI_RB_LAUNCH((hifigan_resblock_kernel<C, K>));
        } else if constexpr (PM == PM_F16) {
            ESMI_RB_LAUNCH((hifigan_resblock_amp_kernel<C, K>));
        } else {
            ESMI_RB_LAUNCH((hifigan_resblock_bf16_kernel<C, K>));
        }
#undef ESMI_RB_LAUNCH
    }
    return launch_status();
}
template <PrecisionMode PM, int C>
int launch_resblock_c(const ResblockP& p, hipStream_t st) {
    switch (p.k) {
        case 3: return launch_resblock_ck<PM, C, 3>(p, st);
        case 7: return launch_resblock_ck<PM, C, 7>(p, st);
        case 11: return launch_resblock_ck<PM, C, 11>(p, st);
    }
    return ESMI_ERR_UNSUPPORTED;
}
template <PrecisionMode PM>
int launch_resblock(const ResblockP& p, int c, hipStream_t st) {
    if constexpr (precision_mode_built(PM)) {
        switch (c) {
            case 8: return launch_resblock_c<PM, 8>(p, st);
            case 16: return launch_resblock_c<PM, 16>(p, st);
            case 32: return launch_resblock_c<PM, 32>(p, st);
            case 64: return launch_resblock_c<PM, 64>(p, st);
        }
    }
    return ESMI_ERR_UNSUPPORTED;
}
// Each mode's twelve kernels compile in a unit of their own, side by side (ESMI_RESBLOCK_INSTANCE): tu_hifigan.hip, which also holds the
// generator's host side (esmi_hifigan_*), tu_hifigan_amp.hip and tu_hifigan_bf16.hip.  No other unit instantiates the ladder:
extern template int launch_resblock<PM_SPLIT>(const ResblockP&, int, hipStream_t);
extern template int launch_resblock<PM_F16>(const ResblockP&, int, hipStream_t);
extern template int launch_resblock<PM_BF16>(const ResblockP&, int, hipStream_t);
#define ESMI_RESBLOCK_INSTANCE(PM) namespace esmi { template int launch_resblock<PM>(const ResblockP&, int, hipStream_t); }

// Does enc_attn_ffn serve this block (the shapes it is instantiated for)?  Not beyond 128 positions: there the chain kernel runs one
// latency chain per 32 rows against up to 256 keys, and the same ops as launches (LDS-staged attention + GEMMs) are faster (launches
// vs chain: small ES at T = 256 2.53 vs 2.62 ms/step, base ES block 0 at N = 256, B = 512 1.33 vs 2.00 ms; tools/debug_plan_base.py).
inline bool enc_attn_ffn_supported(int C, int N, int expansion) {
    if ((C & 31) || N > 128 || N < 1) return false;
    const int nc = C / 32;
    return (expansion == 1 && (nc == 1 || nc == 2 || nc == 4)) || (expansion == 2 && nc == 4);
}

// ---- activation-range check (esmi_dev.h, the ESMI_RANGE_CHECK build): every translation unit owns a copy of the device-side flag
// pointer.  ESMI_TU_RANGE_SETTER(<unit>) links the unit's setter into g_range_setters while the library loads (the head is constant-
// initialised, so the order in which the units' nodes are constructed does not matter); the validation mode of
// esmi_phoneme2mel_forward_curve_f32 (esmi_abi.hip) walks the list.  A unit with kernels that leaves the macro out is not range-checked.
struct RangeSetter;
extern RangeSetter* g_range_setters;   // esmi_abi.hip
struct RangeSetter {
    const char* unit;
    int (*set)(int* flag);
    RangeSetter* next;
    RangeSetter(const char* unit_, int (*set_)(int*)) : unit(unit_), set(set_), next(g_range_setters) { g_range_setters = this; }
};
#if !ESMI_RANGE_CHECK
inline int store_range_flag_pointer(int*) { return ESMI_OK; }   // (the unchecked builds have no flag to point at)
#endif
#define ESMI_TU_RANGE_SETTER(tu) namespace esmi { namespace { RangeSetter range_setter_##tu(#tu, store_range_flag_pointer); } }
// development (-DESMI_CHAIN_TRACE): every translation unit with chain kernels owns a copy of the trace pointer
#ifdef ESMI_CHAIN_TRACE
#define ESMI_TU_CHAIN_TRACE_SETTER(tu) extern "C" void esmi_dev_set_chain_trace_##tu(long long* ptr) { \
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_chain_trace_dev), &ptr, sizeof(ptr)); }
#else
#define ESMI_TU_CHAIN_TRACE_SETTER(tu)
#endif

}  // namespace esmi
#endif  // ESMI_LAUNCH_H
