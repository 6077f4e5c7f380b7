// esmi C-ABI: the host-side launch sequences behind include/esmi.h.
// Built by `hipcc --offload-arch=gfx950` into libesmi.so (product) and, unchanged, by the host
// clang++ with -DESMI_WAVESIM into libesmi_sim.so (CPU wave simulator used only by tests).
#include "launch.h"
#include "dec_layout.h"   // the decoder's build knob (esmi_build_config) and host-side helpers

using namespace esmi;
namespace esmi { RangeSetter* g_range_setters = nullptr; }   // every unit's ESMI_TU_RANGE_SETTER node (launch.h)
ESMI_TU_RANGE_SETTER(abi)

namespace {

// can the mel decoder's first stage run as its own phoneme-rate GEMM launch (esmi_decoder_head_f32)?
bool head_gemm_ok(const esmi_decoder_head* head) {
    return head && head->proj_w && head->proj_b && head->ln_g && head->ln_b && head->d4 > 0 && (head->d4 & 7) == 0 &&
           (head->dx2 == 32 || head->dx2 == 64 || head->dx2 == 128 || head->dx2 == 256);
}

struct EncWs {
    size_t t_merge, qkv, ctx, y1, m1, m2, pmask, total;
};
EncWs enc_ws(const esmi_encoder_block_shape* s) {
    const int n = conv_out_len(s->n_in, s->kernel, s->stride, s->kernel / 2);
    const size_t rows = (size_t)s->B * n;
    EncWs w;
    size_t o = 0;
    w.t_merge = o; o += align256(rows * s->c_in * 4);
    w.qkv = o; o += align256(rows * 3 * s->heads * s->c_out * 4);
    w.ctx = o; o += align256(rows * s->heads * s->c_out * 4);
    w.y1 = o; o += align256(rows * s->c_out * 4);
    w.m1 = o; o += align256(rows * s->c_out * s->expansion * 4);
    w.m2 = o; o += align256(rows * s->c_out * s->expansion * 4);
    w.pmask = o; o += align256(rows);
    w.total = o;
    return w;
}

// ---- the prosody controls (include/esmi.h esmi_prosody_control / esmi_prosody_curves)
// a prosody scale or curve next to the teacher / forced values of the same quantity: the caller asked for two things at once
bool ctl_conflict(const esmi_prosody_curves* ctl, const void* pitch_t, const void* energy_t, const void* dur_t) {
    return ctl && ((ctl->pitch_scale && pitch_t) || (ctl->energy_scale && energy_t) || (ctl->duration_scale && dur_t));
}
// the per-utterance struct as the general one: every pointer is (B).  A temporary of it lives to the end of the forwarding statement
struct PerUtterance {
    esmi_prosody_curves c{};
    explicit PerUtterance(const esmi_prosody_control* ctl) {
        if (ctl) { c.pitch_scale = ctl->pitch_scale; c.energy_scale = ctl->energy_scale; c.duration_scale = ctl->duration_scale; }
    }
    const esmi_prosody_curves* curves() const { return &c; }
};
// What the deciding kernels get (enc_params.h FuseVaP::curve, va_decide.h va_row_scale), written into their parameters: P is FuseVaP,
// Pred128P or VaTailP, which name these seven fields alike.  A (B, T) curve and the teacher / forced array of its quantity are mutually
// exclusive (ctl_conflict), and every kernel loads that array's entry per row anyway: the curve takes the array's place, its kCurve* bit
// says so, and the quantity's (B) scale is absent.
template <class P>
void set_va_controls(P* p, const esmi_prosody_curves& c, const float* pitch_t, const float* energy_t, const int32_t* dur_t) {
    p->pitch_t = pitch_t; p->energy_t = energy_t; p->dur_t = dur_t;
    p->pitch_s = c.pitch_scale; p->energy_s = c.energy_scale; p->dur_s = c.duration_scale; p->curve = 0;
    if (c.pitch_scale && c.pitch_per_phoneme) { p->pitch_t = c.pitch_scale; p->pitch_s = nullptr; p->curve |= kCurvePitch; }
    if (c.energy_scale && c.energy_per_phoneme) { p->energy_t = c.energy_scale; p->energy_s = nullptr; p->curve |= kCurveEnergy; }
    if (c.duration_scale && c.duration_per_phoneme) {
        p->dur_t = reinterpret_cast<const int32_t*>(c.duration_scale); p->dur_s = nullptr; p->curve |= kCurveDur;
    }
}

}  // namespace

#ifdef ESMI_CHAIN_TRACE   // development: tools/trace_chain.py
extern "C" {
void esmi_dev_set_chain_trace_enc_attn_ffn(long long*);
void esmi_dev_set_chain_trace_enc_block(long long*);
void esmi_dev_set_chain_trace_enc_fuse_va(long long*);
void esmi_dev_set_chain_trace_enc_merge(long long*);
void esmi_dev_set_chain_trace(long long* ptr) {
    esmi_dev_set_chain_trace_enc_attn_ffn(ptr); esmi_dev_set_chain_trace_enc_block(ptr);
    esmi_dev_set_chain_trace_enc_fuse_va(ptr); esmi_dev_set_chain_trace_enc_merge(ptr);
}
}
#endif

extern "C" {

int esmi_version(void) { return ESMI_VERSION; }
const char* esmi_backend(void) { return kBackendName; }

const char* esmi_build_config(void) {
#if ESMI_CHAIN_SPLIT
#define ESMI_CFG_ENC_ ",enc_gemm=split-f16x2"
#else
#define ESMI_CFG_ENC_ ",enc_gemm=fp32-mfma"
#endif
#if ESMI_RANGE_CHECK
#define ESMI_CFG_RC_ ",range_check=1"
#else
#define ESMI_CFG_RC_ ""
#endif
    // ... and the compiler the library was built with: two of the chain kernels' forms are work-arounds validated on ROCm 7.2.0's hipcc
    // (chain16.h swap16_f: the select form of v_permlane16_swap; the DPP / ds_swizzle scheduling fence of the fallback LayerNorm,
    // profiles/r05_probes/fuse_va_wrong_rows.md) -- _lib.load() warns when this differs from the validated version
#define ESMI_STR2_(x) #x
#define ESMI_STR_(x) ESMI_STR2_(x)
#if defined(__clang_major__)
#define ESMI_CFG_CC_ ",clang=" ESMI_STR_(__clang_major__) "." ESMI_STR_(__clang_minor__) "." ESMI_STR_(__clang_patchlevel__)
#else
#define ESMI_CFG_CC_ ""
#endif
#if defined(HIP_VERSION_MAJOR)
#define ESMI_CFG_HIP_ ",hip=" ESMI_STR_(HIP_VERSION_MAJOR) "." ESMI_STR_(HIP_VERSION_MINOR) "." ESMI_STR_(HIP_VERSION_PATCH)
#else
#define ESMI_CFG_HIP_ ""
#endif
#if ESMI_DEC_SPLIT == 2
    return "dec_gemm=split-f16x2" ESMI_CFG_ENC_ ESMI_CFG_RC_ ESMI_CFG_HIP_ ESMI_CFG_CC_;
#else
    return "dec_gemm=fp32-mfma" ESMI_CFG_ENC_ ESMI_CFG_RC_ ESMI_CFG_HIP_ ESMI_CFG_CC_;
#endif
}

int esmi_pack_conv_weight_f32(const float* src, float* dst, int cout, int cin, int k, esmi_stream_t stream) {
    if (!src || !dst || cout <= 0 || cin <= 0 || k <= 0) return ESMI_ERR_ARG;
    const long n = (long)cout * cin * k;
    ESMI_LAUNCH(pack_conv_kernel, dim3(grid1d(n)), dim3(256), 0, S(stream), src, dst, cout, cin, k, 0);
    return launch_status();
}
int esmi_pack_convT_weight_f32(const float* src, float* dst, int cin, int cout, int k, esmi_stream_t stream) {
    if (!src || !dst || cout <= 0 || cin <= 0 || k <= 0) return ESMI_ERR_ARG;
    const long n = (long)cout * cin * k;
    ESMI_LAUNCH(pack_conv_kernel, dim3(grid1d(n)), dim3(256), 0, S(stream), src, dst, cout, cin, k, 1);
    return launch_status();
}

size_t esmi_pack_bfrag_floats(int n, int k, int taps) {
    if (n <= 0 || k <= 0 || taps <= 0 || (k & 7)) return 0;
    return (size_t)taps * k * 32 * ((n + 31) / 32);
}
int esmi_pack_bfrag_f32(const float* src, float* dst, int n, int k, int taps, esmi_stream_t stream) {
    if (!src || !dst || n <= 0 || k <= 0 || taps <= 0 || (k & 7)) return ESMI_ERR_ARG;
#if ESMI_CHAIN_SPLIT
    if (k & 31) return ESMI_ERR_UNSUPPORTED;   // the split-f16 packing works on groups of 32 channels (two 16-channel MFMA steps)
#endif
    const long tot = (long)esmi_pack_bfrag_floats(n, k, taps);
    ESMI_LAUNCH(pack_bfrag_kernel, dim3(grid1d(tot)), dim3(256), 0, S(stream), src, dst, n, k, (n + 31) / 32, taps);
    return launch_status();
}

int esmi_compose_merge_f32(const float* merge_w, const float* merge1_w, int k, int cin, int cout, float* dst,
                           esmi_stream_t stream) {
    if (!merge_w || !merge1_w || !dst || k <= 0 || cin <= 0 || cout <= 0) return ESMI_ERR_ARG;
    const long n = (long)k * cin * cout;
    ESMI_LAUNCH(compose_merge_kernel, dim3(grid1d(n)), dim3(256), 0, S(stream), merge_w, merge1_w, dst, k, cin, cout);
    return launch_status();
}

int esmi_pool_mask_u8(const uint8_t* mask, int B, int T, int pool, uint8_t* out, int n_out, esmi_stream_t stream) {
    if (!mask || !out || B <= 0 || T <= 0 || pool <= 0 || n_out <= 0) return ESMI_ERR_ARG;
    ESMI_LAUNCH(pool_mask_kernel, dim3(grid1d(B * n_out)), dim3(256), 0, S(stream), mask, B, T, pool, out, n_out);
    return launch_status();
}

size_t esmi_encoder_block_workspace_bytes(const esmi_encoder_block_shape* s) { return s ? enc_ws(s).total : 0; }

// ------------------------------------------------------------------ encoder side: which kernel serves which shape
// Each stage tries its candidates best first; a launcher answers ESMI_ERR_UNSUPPORTED for a shape it is not built for and the next
// candidate runs.  What serves the published models under launch plan 63:
//   stage                     candidates, in order                               serves
//   whole encoder side        enc_all16 (one-call forward)                       tiny ES (dim 32, MixFFN expansion 1), T <= 128
//   block, whole              enc_block16 > enc_block                            tiny ES blocks (module path); small ES block 0, N <= 128
//   block, front              enc_merge_q256 > enc_merge_qkv > per-op            base ES block 1 > every other packed block
//   block, back               enc_attn_ffn (chosen with the front, N <= 128)     small ES block 1; base ES block 0, N <= 128
//                             attention, then enc_post_attn64 | enc_post_attn128 small ES block 0 | base ES block 0, 128 < N <= 256
//                             > per-op GEMMs                                     base ES block 1; tiny ES block 0 at T > 128; N > 256
//   Fuse + variance adaptor   enc_va16 > enc_va64 > enc_fuse_va                  tiny ES (dim 32) > small ES (dim 64), T <= 256 > longer
//                             enc_fuse128, enc_pred128 > per-op                  base ES (dim 128), T <= 256 > everything else
// A candidate that cannot serve the shape leaves the stage to the next one; any other return code ends the call.
#define ESMI_TRY(eligible, launch)                            \
    if (eligible) {                                           \
        const int rc_ = (launch);                             \
        if (rc_ != ESMI_ERR_UNSUPPORTED) return rc_;          \
    }

namespace {

bool ffn_folded(const esmi_encoder_block_weights* w) { return w->ffn_cw && w->ffn_cwp && w->ffn_cb && w->ffn_cb_first && w->ffn_cb_last; }
// the pre-split weights the chain kernels of a block read (merge convs composed, q / k / v, projection, folded MixFFN, mlp2)
bool block_packed(const esmi_encoder_block_weights* w) { return w->merge_cwp && w->qkv_wp && w->proj_wp && ffn_folded(w) && w->mlp2_wp; }

// The chain kernels' parameters of one block: the merge / qkv stage (f.m) and everything behind the attention.  x_mid / qkv: the block
// input after the merge convs and the q / k / v rows when they travel between two launches (nullptr when one launch does the block).
EncAttnFfnP block_params(const esmi_encoder_block_weights* w, const esmi_encoder_block_shape* s, const int32_t* ids, const float* embed,
                         const float* x_in, const uint8_t* mask, float* x_mid, float* qkv, float* x_out) {
    const int n = conv_out_len(s->n_in, s->kernel, s->stride, s->kernel / 2);
    EncAttnFfnP f;
    memset(&f, 0, sizeof f);
    EncMergeP& m = f.m;
    m.ids = ids; m.table = embed; m.vocab = s->vocab; m.x_in = ids ? nullptr : x_in;
    m.B = s->B; m.n_in = s->n_in; m.n_out = n; m.k = s->kernel; m.stride = s->stride; m.pad = s->kernel / 2; m.h = s->heads;
    m.merge_w = w->merge_cwp; m.qkv_w = w->qkv_wp; m.x_out = x_mid; m.qkv = qkv; m.emb_conv = ids ? w->emb_conv : nullptr;
    m.tiles_per_b = (n + 31) / 32;
    f.x = x_mid; f.qkv = qkv; f.B = s->B; f.N = n; f.C = s->c_out; f.h = s->heads; f.scale = 1.0f / sqrtf((float)(s->c_out / s->heads));
    f.proj_w = w->proj_wp; f.proj_b = w->proj_b; f.ln1_g = w->ln1_g; f.ln1_b = w->ln1_b;
    f.ffn_w = w->ffn_cwp; f.ffn_b = w->ffn_cb; f.ffn_b0 = w->ffn_cb_first; f.ffn_b2 = w->ffn_cb_last;
    f.mlp2_w = w->mlp2_wp; f.mlp2_b = w->mlp2_b; f.ln2_g = w->ln2_g; f.ln2_b = w->ln2_b;
    f.mask = mask; f.out = x_out;
    f.mask_pool = s->mask_pool > 0 ? s->mask_pool : 1; f.mask_len = s->mask_pool > 0 ? s->mask_len : n;
    return f;
}
// ... with the whole-block kernels' weight-folded attention: a third of the q / k / v contraction
void fold_attention(const esmi_encoder_block_weights* w, EncAttnFfnP* f) {
    f->fold = 1; f->m.qkv_w = w->qk_wp; f->m.nq_override = 0; f->proj_w = w->vo_wp;
}

// ---- the one-kernel-per-op plan: the ops that have two callers, then the stages of a block that run when no chain kernel serves them
// the unfolded MixFFN up to its GELU, blocks.py:23-27: mlp1, then the dense k = 3 conv + exact-erf GELU.  x -> m1 -> m2, both (rows, E)
int launch_mixffn_front(int B, int n, int C, int E, const float* x, ConvW mlp1, const float* mlp1_b, ConvW conv, const float* conv_b,
                        float* m1, float* m2, hipStream_t st) {
    if (int rc = launch_convgemm(linear(B, n, C, E, x, C, mlp1, mlp1_b, m1, E), st)) return rc;
    ConvGemmP p = conv1d(B, n, E, E, 3, 1, m1, E, conv, conv_b, m2, E);
    p.act = ACT_GELU;
    return launch_convgemm(p, st);
}

// One predictor (AcousticDecoder, networks.py:148-160) in two launches: conv1 + ReLU -> LN1 -> ReLU into t1 (rows, dim); conv2 + ReLU
// with pred = Linear(dim, 1) on the PRE-norm2 tensor in the epilogue.  `features` (the duration predictor): the prediction passes a
// ReLU and LN2 of the conv2 rows goes to features + row . ldf + f_coff, masked rows zeroed; nullptr: the rows are not stored.
int launch_predictor(const esmi_predictor_weights* w, int dim, int B, int T, const float* x, int ldx, float* t1, float* pred, float* features,
                     int ldf, int f_coff, const uint8_t* mask, hipStream_t st) {
    ConvGemmP p = conv1d(B, T, dim, dim, 3, 1, x, ldx, {w->conv1_w, w->conv1_wp}, w->conv1_b, t1, dim);   // :152-155
    p.act = ACT_RELU; p.ln_g = w->ln1_g; p.ln_b = w->ln1_b; p.post_relu = 1;
    if (int rc = launch_convgemm(p, st)) return rc;
    p = conv1d(B, T, dim, dim, 3, 1, t1, dim, {w->conv2_w, w->conv2_wp}, w->conv2_b, features, features ? ldf : 0);   // :157-160
    p.act = ACT_RELU; p.dot_w = w->lin_w; p.dot_b = w->lin_b; p.dot_out = pred; p.dot_relu = features != nullptr;
    if (features) { p.ln_g = w->ln2_g; p.ln_b = w->ln2_b; p.rowmask = mask; p.o_coff = f_coff; }
    return launch_convgemm(p, st);
}

// the length regulator's scan: cum = the running sum of an utterance's durations, mel_len its total (lmax, optional: the batch's maximum)
void launch_length_regulate(const int32_t* dur, int B, int T, int32_t* cum, int32_t* mel_len, int32_t* lmax, hipStream_t st) {
    ESMI_LAUNCH(length_regulate_kernel, dim3(B), dim3(64), 0, st, dur, T, cum, mel_len, lmax);
}

// front: merge convs + the q / k / v GEMM (folded: q = x M, h*C wide, esmi.h) -> x_mid, qkv
int per_op_front(const esmi_encoder_block_weights* w, const esmi_encoder_block_shape* s, int n, const int32_t* ids, const float* embed,
                 const float* x_in, bool folded, float* t_merge, float* x_mid, float* qkv, hipStream_t st) {
    const int B = s->B, C = s->c_out, nq = (folded ? 1 : 3) * s->heads * C;
    int rc;
    // merge conv k x k (dense, bias-free), networks.py:64-66
    ConvGemmP p = conv_defaults();
    p.B = B; p.n_in = s->n_in; p.c_in = s->c_in; p.n_out = n; p.c_out = s->c_in;
    p.k = s->kernel; p.stride = s->stride; p.pad = s->kernel / 2;
    if (ids) { p.ids = ids; p.table = embed; p.ld_table = s->c_in; p.vocab = s->vocab; }
    else { p.A = x_in; p.lda = s->c_in; }
    if (ESMI_CHAIN_SPLIT && w->merge_cwp && (s->c_in & 31) == 0) {   // (the exact-fp32 build's GEMMs read fp32 weights)
        // both merge convolutions as ONE launch on the composed, pre-split weights the chain kernels use (merge_cwp: k x k conv . 1x1,
        // esmi_compose_merge_f32 -> esmi_pack_bfrag_f32): no t_merge round trip, no weight split per wave
        p.c_out = C; p.W = nullptr; p.Wp = w->merge_cwp; p.out = x_mid; p.ldo = C;
        if ((rc = launch_convgemm(p, st))) return rc;
    } else {
        p.W = w->merge_w; p.out = t_merge; p.ldo = s->c_in;
        if ((rc = launch_convgemm(p, st))) return rc;
        // merge 1x1, networks.py:67
        if ((rc = launch_convgemm(linear(B, n, s->c_in, C, t_merge, s->c_in, {w->merge1_w, nullptr}, nullptr, x_mid, C), st))) return rc;
    }
    // qkv Linear (bias-free), blocks.py:44
    const ConvW qkv_w = folded ? ConvW{w->qk_w, w->qk_wp} : ConvW{w->qkv_w, w->qkv_wp};
    return launch_convgemm(linear(B, n, C, nq, x_mid, C, qkv_w, nullptr, qkv, nq), st);
}

// softmax(q k^T scale) v -> ctx, blocks.py:49-64 (scores not masked).  qkv: the q | k | v rows; folded: q_h = x M_h, h*C wide, and
// keys = values = x, shared by the heads
int launch_self_attention(int B, int n, int C, int h, bool folded, float* qkv, float* x, float* ctx, hipStream_t st) {
    AttnP a = {};
    a.B = B; a.N = n; a.C = C; a.h = h; a.ctx = ctx; a.scale = 1.0f / sqrtf((float)(C / h));
    if (!folded) a.qkv = qkv;
    else { a.q = qkv; a.ldq = h * C; a.hsq = C; a.k = a.v = x; a.ldk = a.ldv = C; a.hsk = a.hsv = 0; }
    return launch_attn(a, st);
}

// back, behind the attention: proj + LN1, MixFFN, mlp2 + LN2 -> x_out.  mask: pooled to the block's (B, n)
int per_op_post_attention(const esmi_encoder_block_weights* w, const esmi_encoder_block_shape* s, int n, bool folded, const uint8_t* mask,
                          const float* ctx, float* y1, float* m1, float* m2, float* x_out, hipStream_t st) {
    const int B = s->B, C = s->c_out, h = s->heads, E = C * s->expansion;
    int rc;
    // proj + residual + LN1 + mask, blocks.py:65 + networks.py:73-75  (folded: ctx holds P_h x, the matrix is [O_h])
    ConvGemmP p = linear(B, n, h * C, C, ctx, h * C, folded ? ConvW{w->vo_w, w->vo_wp} : ConvW{w->proj_w, w->proj_wp}, w->proj_b, y1, C);
    p.res = x_out; p.ldr = C; p.ln_g = w->ln1_g; p.ln_b = w->ln1_b; p.rowmask = mask;
    if ((rc = launch_convgemm(p, st))) return rc;
    // MixFFN, blocks.py:22-29
    if (ffn_folded(w)) {   // Linear folded into the k = 3 conv (esmi.h, ffn_cw): one contraction C -> E, position-dependent bias at the two ends
        p = conv1d(B, n, C, E, 3, 1, y1, C, {w->ffn_cw, w->ffn_cwp}, w->ffn_cb, m2, E);
        p.bias_first = w->ffn_cb_first; p.bias_last = w->ffn_cb_last; p.act = ACT_GELU;
        rc = launch_convgemm(p, st);
    } else {
        rc = launch_mixffn_front(B, n, C, E, y1, {w->mlp1_w, w->mlp1_wp}, w->mlp1_b, {w->conv_w, w->conv_wp}, w->conv_b, m1, m2, st);
    }
    if (rc) return rc;
    // mlp2 + residual + LN2 + mask, networks.py:80-83
    p = linear(B, n, E, C, m2, E, {w->mlp2_w, w->mlp2_wp}, w->mlp2_b, x_out, C);
    p.res = y1; p.ldr = C; p.ln_g = w->ln2_g; p.ln_b = w->ln2_b; p.rowmask = mask;
    return launch_convgemm(p, st);
}

}  // namespace

int esmi_encoder_block_f32(const esmi_encoder_block_weights* w, const esmi_encoder_block_shape* s, const int32_t* ids,
                           const float* embed, const float* x_in, const uint8_t* mask, float* x_out, void* workspace,
                           size_t workspace_bytes, esmi_stream_t stream) {
    if (!w || !s || !x_out || !workspace) return ESMI_ERR_ARG;
    if (!ids && !x_in) return ESMI_ERR_ARG;
    const int plan = s->plan & ESMI_FUSE_ALL;
    const bool chain16 = plan & ESMI_FUSE_CHAIN16;
    const EncWs ws = enc_ws(s);
    if (workspace_bytes < ws.total) return ESMI_ERR_WORKSPACE;
    char* wsb = static_cast<char*>(workspace);
    auto F = [&](size_t off) { return reinterpret_cast<float*>(wsb + off); };
    const int B = s->B, C = s->c_out, h = s->heads;
    const int n = conv_out_len(s->n_in, s->kernel, s->stride, s->kernel / 2);
    hipStream_t st = S(stream);
    const bool packed = block_packed(w);
    // enc_attn_ffn behind the front: x (the block input after the merge convs) lives in scratch and the result goes straight to x_out
    // (tiles read their neighbours' x rows, so in place is not possible)
    const bool attn_ffn = packed && (plan & ESMI_FUSE_ATTN_FFN) && enc_attn_ffn_supported(C, n, s->expansion);
    // one-kernel-per-op attention with folded weights (esmi.h): the Linear behind the merge convs is x M (h*C wide) instead of qkv
    const bool folded = !attn_ffn && h >= 2 && w->qk_w && w->qk_wp && w->vo_w && w->vo_wp;   // (one head: measured no gain per op; HISTORY.md 3.3)
    float *qkv = F(ws.qkv), *ctx = F(ws.ctx), *y1 = F(ws.y1), *x_mid = attn_ffn ? y1 : x_out;
    const EncAttnFfnP f = block_params(w, s, ids, embed, x_in, mask, x_mid, qkv, x_out);

    // ---- the whole block in one launch
    if (attn_ffn && (plan & ESMI_FUSE_MERGE_QKV) && (plan & ESMI_FUSE_BLOCK)) {
        EncAttnFfnP fb = f;
        fb.x = nullptr; fb.qkv = nullptr;
        if (w->qk_wp && w->vo_wp) fold_attention(w, &fb);
        ESMI_TRY(chain16, launch_enc_block16(fb, s->expansion, s->c_in, st))
        ESMI_TRY(true, launch_enc_block(fb, s->expansion, s->c_in, plan & ESMI_FUSE_SPLIT2, st))
    }

    // ---- front: merge convs + the q / k / v GEMM (folded: q) -> x_mid, qkv
    auto front = [&]() -> int {
        ESMI_TRY(chain16 && folded && !ids && x_in && s->c_in == 128 && C == 256 && s->stride == 2 && n <= 128 && w->merge_cwp,
                 launch_enc_merge_q256(MergeQ256P{x_in, x_mid, qkv, w->merge_cwp, w->qk_wp, B, s->n_in, n, s->kernel, h}, st))
        if (packed && (plan & ESMI_FUSE_MERGE_QKV)) {
            EncMergeP m = f.m;
            if (folded) { m.qkv_w = w->qk_wp; m.nq_override = h * C; }
            ESMI_TRY(true, launch_enc_merge_qkv(m, s->c_in, C, st))
        }
        return per_op_front(w, s, n, ids, embed, x_in, folded, F(ws.t_merge), x_mid, qkv, st);
    };
    if (int rc = front()) return rc;

    // ---- back: attention + proj + LN1 + MixFFN + LN2 -> x_out
    if (attn_ffn) return launch_enc_attn_ffn(f, s->expansion, plan & ESMI_FUSE_SPLIT2, st);   // (the front wrote x to y1 for it)
    if (mask && s->mask_pool > 1) {   // the one-kernel-per-op plan takes a pooled (B, n) mask: blocks.py:51-57
        uint8_t* pm = reinterpret_cast<uint8_t*>(wsb + ws.pmask);
        if (int rc = esmi_pool_mask_u8(mask, B, s->mask_len, s->mask_pool, pm, n, stream)) return rc;
        mask = pm;
    }
    if (int rc = launch_self_attention(B, n, C, h, folded, qkv, x_out, ctx, st)) return rc;
    // everything behind the attention in one launch; folded (enc_ffn128.h): ctx = the heads' P_h x, the projection is [Wv_h^T Wp_h^T]
    ESMI_TRY(chain16 && packed && !folded && C == 64 && h == 1 && s->expansion == 1 && n <= 256,
             launch_enc_post_attn64(PostAttn64P{ctx, x_out, x_out, w->proj_wp, w->ffn_cwp, w->mlp2_wp, w->proj_b, w->ln1_g, w->ln1_b, w->ffn_cb,
                                                w->ffn_cb_first, w->ffn_cb_last, w->mlp2_b, w->ln2_g, w->ln2_b, mask, B, n}, st))
    ESMI_TRY(chain16 && packed && folded && C == 128 && h == 2 && s->expansion == 2 && n <= 256,
             launch_enc_post_attn128(PostAttn128P{ctx, x_out, y1, x_out, w->vo_wp, w->ffn_cwp, w->mlp2_wp, w->proj_b, w->ln1_g, w->ln1_b,
                                                  w->ffn_cb, w->ffn_cb_first, w->ffn_cb_last, w->mlp2_b, w->ln2_g, w->ln2_b, mask, B, n}, st))
    return per_op_post_attention(w, s, n, folded, mask, ctx, y1, F(ws.m1), F(ws.m2), x_out, st);
}

size_t esmi_fuse_workspace_bytes(int B, int T, int dim, int depth) {
    return align256((size_t)B * T * dim * depth * 4) + align256((size_t)B * T * dim * 4);
}

int esmi_fuse_f32(const esmi_fuse_weights* w, int depth, int dim, int kernel, int B, int T, const float* const* feats,
                  const int* n_i, const uint8_t* mask, float* out, int ld_out, void* workspace, size_t workspace_bytes,
                  esmi_stream_t stream) {
    if (!w || !feats || !n_i || !out || !workspace || depth < 1 || depth > ESMI_MAX_DEPTH) return ESMI_ERR_ARG;
    if (workspace_bytes < esmi_fuse_workspace_bytes(B, T, dim, depth)) return ESMI_ERR_WORKSPACE;
    float* cat = static_cast<float*>(workspace);
    float* tmp = reinterpret_cast<float*>(static_cast<char*>(workspace) + align256((size_t)B * T * dim * depth * 4));
    hipStream_t st = S(stream);
    int rc;
    for (int i = 0; i < depth; ++i) {
        const int ci = dim << i, s = 1 << i;
        if (i == 0 && n_i[0] != T) return ESMI_ERR_ARG;
        // Linear(dim*2^i, dim), networks.py:197: level 0 straight into its columns of the concatenation
        ConvGemmP p = linear(B, n_i[i], ci, dim, feats[i], ci, {w->mlp_w[i], w->mlp_wp[i]}, w->mlp_b[i], i == 0 ? cat : tmp, i == 0 ? dim * depth : dim);
        if ((rc = launch_convgemm(p, st))) return rc;
        if (i == 0) continue;
        if ((n_i[i] - 1) * s + kernel < T) return ESMI_ERR_UNSUPPORTED;  // torch.cat would raise in the reference
        // ConvTranspose1d(dim, dim, k, stride 2^i) cropped to T, networks.py:199-206  (the streaming kernel reads the pre-split blob: round 5)
        p = conv_transpose1d(B, n_i[i], T, dim, dim, kernel, s, 0, tmp, dim, {w->up_w[i], w->up_wp[i]}, w->up_b[i], cat, dim * depth);
        p.o_coff = i * dim;
        if ((rc = launch_convgemm(p, st))) return rc;
    }
    // Linear(depth*dim, dim) + masked_fill, networks.py:215-217
    ConvGemmP p = linear(B, T, dim * depth, dim, cat, dim * depth, {w->fuse_w, w->fuse_wp}, w->fuse_b, out, ld_out);
    p.rowmask = mask;
    return launch_convgemm(p, st);
}

size_t esmi_variance_adaptor_workspace_bytes(int B, int T, int dim) { return align256((size_t)B * T * dim * 4); }

int esmi_variance_adaptor_f32(const esmi_predictor_weights* pitch, const esmi_predictor_weights* energy,
                              const esmi_predictor_weights* duration, int dim, int B, int T, const uint8_t* mask,
                              const float* pitch_target, const float* energy_target, const int32_t* duration_target,
                              float* feat, float* pitch_pred, float* energy_pred, float* duration_pred,
                              int32_t* pitch_idx, int32_t* energy_idx, int32_t* dur, void* workspace,
                              size_t workspace_bytes, esmi_stream_t stream) {
    return esmi_variance_adaptor_curve_f32(pitch, energy, duration, dim, B, T, mask, pitch_target, energy_target, duration_target, feat, pitch_pred,
                                           energy_pred, duration_pred, pitch_idx, energy_idx, dur, workspace, workspace_bytes, stream, nullptr);
}

int esmi_variance_adaptor_ctl_f32(const esmi_predictor_weights* pitch, const esmi_predictor_weights* energy,
                                  const esmi_predictor_weights* duration, int dim, int B, int T, const uint8_t* mask,
                                  const float* pitch_target, const float* energy_target, const int32_t* duration_target,
                                  float* feat, float* pitch_pred, float* energy_pred, float* duration_pred,
                                  int32_t* pitch_idx, int32_t* energy_idx, int32_t* dur, void* workspace,
                                  size_t workspace_bytes, esmi_stream_t stream, const esmi_prosody_control* ctl) {
    return esmi_variance_adaptor_curve_f32(pitch, energy, duration, dim, B, T, mask, pitch_target, energy_target, duration_target, feat, pitch_pred,
                                           energy_pred, duration_pred, pitch_idx, energy_idx, dur, workspace, workspace_bytes, stream,
                                           PerUtterance(ctl).curves());
}

int esmi_variance_adaptor_curve_f32(const esmi_predictor_weights* pitch, const esmi_predictor_weights* energy,
                                    const esmi_predictor_weights* duration, int dim, int B, int T, const uint8_t* mask,
                                    const float* pitch_target, const float* energy_target, const int32_t* duration_target,
                                    float* feat, float* pitch_pred, float* energy_pred, float* duration_pred,
                                    int32_t* pitch_idx, int32_t* energy_idx, int32_t* dur, void* workspace,
                                    size_t workspace_bytes, esmi_stream_t stream, const esmi_prosody_curves* ctl) {
    if (ctl_conflict(ctl, pitch_target, energy_target, duration_target)) return ESMI_ERR_ARG;
    if (!pitch || !energy || !duration || !feat || !pitch_pred || !energy_pred || !duration_pred || !dur || !workspace)
        return ESMI_ERR_ARG;
    if (workspace_bytes < esmi_variance_adaptor_workspace_bytes(B, T, dim)) return ESMI_ERR_WORKSPACE;
    float* t1 = static_cast<float*>(workspace);
    hipStream_t st = S(stream);
    // the fused features are columns [0, dim) of feat's 4 dim; the duration predictor's features go to [3 dim, 4 dim), masked (:366-368)
    int rc;
    if ((rc = launch_predictor(pitch, dim, B, T, feat, 4 * dim, t1, pitch_pred, nullptr, 0, 0, nullptr, st))) return rc;
    if ((rc = launch_predictor(energy, dim, B, T, feat, 4 * dim, t1, energy_pred, nullptr, 0, 0, nullptr, st))) return rc;
    if ((rc = launch_predictor(duration, dim, B, T, feat, 4 * dim, t1, duration_pred, feat, 4 * dim, 3 * dim, mask, st))) return rc;
    VaTailP v;
    v.rows = B * T; v.T = T; v.dim = dim; v.mask = mask;
    v.pitch_pred = pitch_pred; v.energy_pred = energy_pred; v.dur_pred = duration_pred;
    set_va_controls(&v, ctl ? *ctl : esmi_prosody_curves{}, pitch_target, energy_target, duration_target);
    v.pbins = pitch->bins; v.ebins = energy->bins; v.pemb = pitch->emb; v.eemb = energy->emb;
    v.feat = feat; v.pitch_idx = pitch_idx; v.energy_idx = energy_idx; v.dur = dur;
    if (!v.pbins || !v.ebins || !v.pemb || !v.eemb) return ESMI_ERR_ARG;
    if (dim & 3) return ESMI_ERR_UNSUPPORTED;                  // (dim = embed_dim // reduction: 32 / 64 / 128 for the published sizes)
    const long n = (long)B * T * (dim >> 2);                   // one thread per four channels
    ESMI_LAUNCH(va_tail_kernel, dim3(grid1d(n)), dim3(256), 0, st, v);
    return launch_status();
}

size_t esmi_fuse_variance_adaptor_workspace_bytes(int B, int T, int dim, int depth) {
    return esmi_fuse_workspace_bytes(B, T, dim, depth) + esmi_variance_adaptor_workspace_bytes(B, T, dim);
}

namespace {

// the Fuse + variance-adaptor stage's arguments (esmi_fuse_variance_adaptor_f32's, and the one-call forward's)
struct VaArgs {
    const esmi_fuse_weights* fw;
    int depth, dim, kernel, B, T;
    const float* const* feats;
    const int* n_i;
    const esmi_predictor_weights* pw[3];   // pitch, energy, duration
    const uint8_t* mask;
    const float *pitch_t, *energy_t;
    const int32_t* dur_t;
    float *feat, *preds[3];
    int32_t *pitch_idx, *energy_idx, *dur, *cum, *mel_len;
    const esmi_decoder_head* head;
    float* h0;
    int plan;
    void* workspace;
    size_t workspace_bytes;
    esmi_stream_t stream;
    // the caller (the one-call inference forward) only consumes duration_pred / dur / cum / mel_len / h0: when a chain kernel produces
    // h0, the phoneme-rate feature tensor, the pitch / energy predictions and the bucket indices are not written at all (16.8 MB of
    // stores per tiny-ES batch that nobody reads: the decoder gathers h0)
    bool lean;
    esmi_prosody_curves ctl;    // (B) scales or (B, T) curves of the predictions that are bucketized / rounded (all NULL: none)
};

// does the fused Fuse + variance-adaptor chain kernel family (enc_va16 / enc_va64 / enc_fuse_va) serve this call?  (packed weights)
bool va_chain_ok(const VaArgs& a) {
    if (!(a.plan & ESMI_FUSE_VARIANCE) || (a.dim != 32 && a.dim != 64) || (a.kernel != 3 && a.kernel != 5) || a.n_i[0] != a.T || !a.fw->fuse_wp)
        return false;
    for (int q = 0; q < 3; ++q)
        if (!a.pw[q]->conv1_wp || !a.pw[q]->conv2_wp) return false;
    for (int i = 0; i < a.depth; ++i)
        if (!a.fw->mlp_wp[i] || (i > 0 && !a.fw->up_wp[i])) return false;
    return true;
}

// Where the mel decoder's first stage runs at phoneme rate: inside the chain kernel (dim 32 models), as its own GEMM launch behind the
// variance adaptor (esmi_decoder_head_f32), or not at all (the decoder runs it at frame rate).
enum class Head { none, in_chain, gemm };
Head phoneme_rate_head(const VaArgs& a, const esmi_decoder_head* head) {
    if (!head) return Head::none;
    if (va_chain_ok(a) && head->proj_wp && a.dim == 32 && head->d4 == 128 && head->dx2 == 128) return Head::in_chain;
    if (head_gemm_ok(head) && head->d4 == 4 * a.dim) return Head::gemm;
    return Head::none;
}

void set_head(FuseVaP* p, const esmi_decoder_head* head, float* h0) {
    p->head_w = head->proj_wp; p->head_b = head->proj_b; p->head_g = head->ln_g; p->head_beta = head->ln_b; p->h0 = h0;
}
void drop_unread_outputs(FuseVaP* p) {   // (VaArgs::lean)
    p->feat = nullptr; p->preds[0] = p->preds[1] = nullptr; p->pitch_idx = p->energy_idx = nullptr;
}

// the Fuse part of the chain kernels' parameters
FuseVaP fuse_params(const VaArgs& a) {
    FuseVaP p;
    memset(&p, 0, sizeof p);
    p.B = a.B; p.T = a.T; p.depth = a.depth; p.kernel = a.kernel;
    for (int i = 0; i < a.depth; ++i) {
        p.feats[i] = a.feats[i]; p.n_i[i] = a.n_i[i];
        p.mlp_w[i] = a.fw->mlp_wp[i]; p.mlp_b[i] = a.fw->mlp_b[i]; p.up_w[i] = a.fw->up_wp[i]; p.up_b[i] = a.fw->up_b[i];
    }
    p.fuse_w = a.fw->fuse_wp; p.fuse_b = a.fw->fuse_b; p.mask = a.mask; p.feat = a.feat;
    return p;
}
void pred_weights(const VaArgs& a, PredW* out) {
    for (int q = 0; q < 3; ++q) {
        const esmi_predictor_weights* w = a.pw[q];
        out[q] = PredW{w->conv1_wp, w->conv1_b, w->ln1_g, w->ln1_b, w->conv2_wp, w->conv2_b, w->ln2_g, w->ln2_b, w->lin_w, w->lin_b, w->bins, w->emb};
    }
}
// ... and the whole parameter block of the Fuse + variance-adaptor chain kernels
FuseVaP va_chain_params(const VaArgs& a, bool head_in_chain, int* nw) {
    FuseVaP p = fuse_params(a);
    pred_weights(a, p.pred);
    set_va_controls(&p, a.ctl, a.pitch_t, a.energy_t, a.dur_t);
    for (int q = 0; q < 3; ++q) p.preds[q] = a.preds[q];
    p.pitch_idx = a.pitch_idx; p.energy_idx = a.energy_idx; p.dur = a.dur;
    fuse_va_plan(a.T, a.dim, a.depth, nw, &p.wgs_per_b, &p.useful, &p.halo);
    const bool scan_fused = a.cum && p.halo == 0;   // one workgroup sees every duration of its utterance
    p.cum = scan_fused ? a.cum : nullptr; p.mel_len = scan_fused ? a.mel_len : nullptr;
    if (head_in_chain) set_head(&p, a.head, a.h0);
    return p;
}

// enc_pred128 DMA-loads every one of these for all three predictors (esmi.h lets a caller leave pitch / energy's ln2 NULL)
bool pred128_weights_ok(const VaArgs& a) {
    for (int q = 0; q < 3; ++q) {
        const esmi_predictor_weights* w = a.pw[q];
        if (!w->conv1_wp || !w->conv1_b || !w->ln1_g || !w->ln1_b || !w->conv2_wp || !w->conv2_b || !w->ln2_g || !w->ln2_b || !w->lin_w || !w->lin_b)
            return false;
    }
    return true;
}

int fuse_variance_adaptor(const VaArgs& a) {
    if (ctl_conflict(&a.ctl, a.pitch_t, a.energy_t, a.dur_t)) return ESMI_ERR_ARG;
    if ((a.cum == nullptr) != (a.mel_len == nullptr)) return ESMI_ERR_ARG;
    if (a.h0 && (!a.head || (!a.head->proj_wp && !a.head->proj_w) || !a.head->proj_b || !a.head->ln_g || !a.head->ln_b)) return ESMI_ERR_ARG;
    if (!a.fw || !a.feats || !a.n_i || !a.pw[0] || !a.pw[1] || !a.pw[2] || !a.feat || !a.preds[0] || !a.preds[1] || !a.preds[2] || !a.dur ||
        a.depth < 1 || a.depth > ESMI_MAX_DEPTH)
        return ESMI_ERR_ARG;
    const Head head = a.h0 ? phoneme_rate_head(a, a.head) : Head::none;
    if (a.h0 && head == Head::none) return ESMI_ERR_UNSUPPORTED;
    const bool head_in_chain = head == Head::in_chain, chain16 = a.plan & ESMI_FUSE_CHAIN16;
    hipStream_t st = S(a.stream);
    bool head_done = head_in_chain;
    int rc;
    if (va_chain_ok(a)) {   // ---- the whole stage in one chain kernel
        for (int i = 1; i < a.depth; ++i)
            if ((a.n_i[i] - 1) * (1 << i) + a.kernel < a.T) return ESMI_ERR_UNSUPPORTED;   // torch.cat would raise in the reference
        if (!a.pw[0]->bins || !a.pw[0]->emb || !a.pw[1]->bins || !a.pw[1]->emb) return ESMI_ERR_ARG;
        int nw;
        const FuseVaP p = va_chain_params(a, head_in_chain, &nw);
        bool scan_done = p.cum != nullptr;
        auto chain = [&]() -> int {
            if (chain16 && scan_done == (a.cum != nullptr)) {
                FuseVaP q = p;
                if (a.lean && head_in_chain) drop_unread_outputs(&q);
                ESMI_TRY(true, launch_enc_va16(q, a.dim, a.kernel, st))
            }
            if (chain16 && !head_in_chain) {
                // dim = 64, T <= 256: one workgroup per utterance, so the length regulator's scan runs inside it -- and the decoder's
                // phoneme-rate first stage too when the caller wants h0 (4 dim = dx2 = 256, pre-split weights)
                FuseVaP q = p;
                q.cum = a.cum; q.mel_len = a.mel_len;
                const bool head64 = a.h0 && a.head->proj_wp && a.head->d4 == 4 * a.dim && a.head->dx2 == 4 * a.dim;
                if (head64) {
                    set_head(&q, a.head, a.h0);
                    if (a.lean) drop_unread_outputs(&q);
                }
                const int rc64 = launch_enc_va64(q, a.dim, a.kernel, st);
                if (rc64 == ESMI_OK) { scan_done = a.cum != nullptr; head_done = head64; }
                if (rc64 != ESMI_ERR_UNSUPPORTED) return rc64;
            }
            return launch_enc_fuse_va(p, a.dim, a.kernel, nw, head_in_chain, st);
        };
        if ((rc = chain())) return rc;
        if (a.cum && !scan_done) launch_length_regulate(a.dur, a.B, a.T, a.cum, a.mel_len, nullptr, st);
    } else {                // ---- Fuse, then the three predictors + the variance adaptor's tail + the length regulator's scan
        if (!a.workspace || a.workspace_bytes < esmi_fuse_variance_adaptor_workspace_bytes(a.B, a.T, a.dim, a.depth)) return ESMI_ERR_WORKSPACE;
        const size_t fws = esmi_fuse_workspace_bytes(a.B, a.T, a.dim, a.depth);
        const esmi_fuse_weights* fw = a.fw;
        auto fuse = [&]() -> int {
            ESMI_TRY(chain16 && a.dim == 128 && a.depth == 2 && fw->mlp_wp[0] && fw->mlp_wp[1] && fw->up_wp[1] && fw->fuse_wp,
                     launch_enc_fuse128(fuse_params(a), a.dim, a.kernel, st))
            return esmi_fuse_f32(fw, a.depth, a.dim, a.kernel, a.B, a.T, a.feats, a.n_i, a.mask, a.feat, 4 * a.dim, a.workspace, fws, a.stream);
        };
        auto predictors = [&]() -> int {
            if (chain16 && a.dim == 128 && pred128_weights_ok(a)) {
                Pred128P q{{}, a.mask, nullptr, nullptr, nullptr, a.feat, {a.preds[0], a.preds[1], a.preds[2]}, a.pitch_idx, a.energy_idx,
                           a.dur, a.cum, a.mel_len, a.B, a.T};
                set_va_controls(&q, a.ctl, a.pitch_t, a.energy_t, a.dur_t);
                pred_weights(a, q.pred);
                ESMI_TRY(true, launch_enc_pred128(q, a.dim, st))
            }
            const int r = esmi_variance_adaptor_curve_f32(a.pw[0], a.pw[1], a.pw[2], a.dim, a.B, a.T, a.mask, a.pitch_t, a.energy_t, a.dur_t, a.feat,
                                                          a.preds[0], a.preds[1], a.preds[2], a.pitch_idx, a.energy_idx, a.dur,
                                                          static_cast<char*>(a.workspace) + fws, a.workspace_bytes - fws, a.stream, &a.ctl);
            if (r) return r;
            if (a.cum) launch_length_regulate(a.dur, a.B, a.T, a.cum, a.mel_len, nullptr, st);
            return ESMI_OK;
        };
        if ((rc = fuse()) || (rc = predictors())) return rc;
    }
    if (a.h0 && !head_done) return esmi_decoder_head_f32(a.head, (long)a.B * a.T, a.feat, a.h0, a.stream);
    return launch_status();
}

}  // namespace

int esmi_fuse_variance_adaptor_f32(const esmi_fuse_weights* fw, int depth, int dim, int kernel, int B, int T,
                                   const float* const* feats, const int* n_i, const esmi_predictor_weights* pitch,
                                   const esmi_predictor_weights* energy, const esmi_predictor_weights* duration,
                                   const uint8_t* mask, const float* pitch_target, const float* energy_target,
                                   const int32_t* duration_target, float* feat, float* pitch_pred, float* energy_pred,
                                   float* duration_pred, int32_t* pitch_idx, int32_t* energy_idx, int32_t* dur,
                                   int32_t* cum, int32_t* mel_len, const esmi_decoder_head* head, float* h0, int plan,
                                   void* workspace, size_t workspace_bytes, esmi_stream_t stream) {
    return esmi_fuse_variance_adaptor_curve_f32(fw, depth, dim, kernel, B, T, feats, n_i, pitch, energy, duration, mask, pitch_target, energy_target,
                                                duration_target, feat, pitch_pred, energy_pred, duration_pred, pitch_idx, energy_idx, dur, cum,
                                                mel_len, head, h0, plan, workspace, workspace_bytes, stream, nullptr);
}

int esmi_fuse_variance_adaptor_ctl_f32(const esmi_fuse_weights* fw, int depth, int dim, int kernel, int B, int T,
                                       const float* const* feats, const int* n_i, const esmi_predictor_weights* pitch,
                                       const esmi_predictor_weights* energy, const esmi_predictor_weights* duration,
                                       const uint8_t* mask, const float* pitch_target, const float* energy_target,
                                       const int32_t* duration_target, float* feat, float* pitch_pred, float* energy_pred,
                                       float* duration_pred, int32_t* pitch_idx, int32_t* energy_idx, int32_t* dur,
                                       int32_t* cum, int32_t* mel_len, const esmi_decoder_head* head, float* h0, int plan,
                                       void* workspace, size_t workspace_bytes, esmi_stream_t stream, const esmi_prosody_control* ctl) {
    return esmi_fuse_variance_adaptor_curve_f32(fw, depth, dim, kernel, B, T, feats, n_i, pitch, energy, duration, mask, pitch_target, energy_target,
                                                duration_target, feat, pitch_pred, energy_pred, duration_pred, pitch_idx, energy_idx, dur, cum,
                                                mel_len, head, h0, plan, workspace, workspace_bytes, stream, PerUtterance(ctl).curves());
}

int esmi_fuse_variance_adaptor_curve_f32(const esmi_fuse_weights* fw, int depth, int dim, int kernel, int B, int T,
                                         const float* const* feats, const int* n_i, const esmi_predictor_weights* pitch,
                                         const esmi_predictor_weights* energy, const esmi_predictor_weights* duration,
                                         const uint8_t* mask, const float* pitch_target, const float* energy_target,
                                         const int32_t* duration_target, float* feat, float* pitch_pred, float* energy_pred,
                                         float* duration_pred, int32_t* pitch_idx, int32_t* energy_idx, int32_t* dur,
                                         int32_t* cum, int32_t* mel_len, const esmi_decoder_head* head, float* h0, int plan,
                                         void* workspace, size_t workspace_bytes, esmi_stream_t stream, const esmi_prosody_curves* ctl) {
    return fuse_variance_adaptor(VaArgs{fw, depth, dim, kernel, B, T, feats, n_i, {pitch, energy, duration}, mask, pitch_target, energy_target,
                                        duration_target, feat, {pitch_pred, energy_pred, duration_pred}, pitch_idx, energy_idx, dur, cum, mel_len,
                                        head, h0, plan, workspace, workspace_bytes, stream, false, ctl ? *ctl : esmi_prosody_curves{}});
}

// MelDecoder's first stage at phoneme rate as one launch: GEMM (k = 1) + bias + tanh + LayerNorm in the epilogue (networks.py:291-293)
int esmi_decoder_head_f32(const esmi_decoder_head* head, long rows, const float* feat, float* h0, esmi_stream_t stream) {
    if (!head_gemm_ok(head) || !feat || !h0 || rows <= 0 || rows > 0x7fffffffL) return head_gemm_ok(head) ? ESMI_ERR_ARG : ESMI_ERR_UNSUPPORTED;
    // (proj_wp, optional: pre-split fragments -- the LDS-staged kernel then brings the weight tiles in by LDS-DMA)
    ConvGemmP p = linear(1, (int)rows, head->d4, head->dx2, feat, head->d4, {head->proj_w, head->proj_wp}, head->proj_b, h0, head->dx2);
    p.act = ACT_TANH; p.ln_g = head->ln_g; p.ln_b = head->ln_b;
    return launch_convgemm(p, S(stream));
}

float esmi_split_weight_limit(void) {
#if ESMI_CHAIN_SPLIT || ESMI_DEC_SPLIT
    return 65504.0f / kF16WScale;   // 2^8 * W must stay a finite binary16 number
#else
    return __builtin_huge_valf();
#endif
}

int esmi_absmax_f32(const float* x, int64_t n, float* out, esmi_stream_t stream) {
    if (!x || !out || n <= 0) return ESMI_ERR_ARG;
    hipError_t e = hipMemsetAsync(out, 0, sizeof(float), S(stream));
    if (e != hipSuccess) return (int)e;
    const long blocks = (n + 256L * 8 - 1) / (256L * 8);
    ESMI_LAUNCH(absmax_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)), dim3(256), 0, S(stream), x, (long)n, reinterpret_cast<int*>(out));
    return launch_status();
}

// ------------------------------------------------------------------ module-level forwards (one kernel per reference op)
size_t esmi_self_attention_workspace_bytes(int B, int N, int C, int heads) {
    if (B <= 0 || N <= 0 || C <= 0 || heads <= 0) return 0;
    const size_t rows = (size_t)B * N;
    return align256(rows * 3 * heads * C * 4) + align256(rows * heads * C * 4);
}

int esmi_self_attention_f32(const float* qkv_w, const float* proj_w, const float* proj_b, int B, int N, int C, int heads,
                            const float* x, float* out, void* workspace, size_t workspace_bytes, esmi_stream_t stream) {
    if (!qkv_w || !proj_w || !proj_b || !x || !out || !workspace || B <= 0 || N <= 0 || C <= 0 || heads <= 0) return ESMI_ERR_ARG;
    if (workspace_bytes < esmi_self_attention_workspace_bytes(B, N, C, heads)) return ESMI_ERR_WORKSPACE;
    float* qkv = static_cast<float*>(workspace);
    float* ctx = reinterpret_cast<float*>(static_cast<char*>(workspace) + align256((size_t)B * N * 3 * heads * C * 4));
    hipStream_t st = S(stream);
    int rc;
    // qkv Linear (bias-free), blocks.py:44
    if ((rc = launch_convgemm(linear(B, N, C, 3 * heads * C, x, C, {qkv_w, nullptr}, nullptr, qkv, 3 * heads * C), st))) return rc;
    if ((rc = launch_self_attention(B, N, C, heads, false, qkv, nullptr, ctx, st))) return rc;
    return launch_convgemm(linear(B, N, heads * C, C, ctx, heads * C, {proj_w, nullptr}, proj_b, out, C), st);   // proj, blocks.py:65
}

size_t esmi_mixffn_workspace_bytes(int B, int N, int C, int expansion) {
    if (B <= 0 || N <= 0 || C <= 0 || expansion <= 0) return 0;
    return 2 * align256((size_t)B * N * C * expansion * 4);
}

int esmi_mixffn_f32(const float* mlp1_w, const float* mlp1_b, const float* conv_w, const float* conv_b, const float* mlp2_w,
                    const float* mlp2_b, int B, int N, int C, int expansion, const float* x, float* out, void* workspace,
                    size_t workspace_bytes, esmi_stream_t stream) {
    if (!mlp1_w || !mlp1_b || !conv_w || !conv_b || !mlp2_w || !mlp2_b || !x || !out || !workspace) return ESMI_ERR_ARG;
    if (B <= 0 || N <= 0 || C <= 0 || expansion <= 0) return ESMI_ERR_ARG;
    if (workspace_bytes < esmi_mixffn_workspace_bytes(B, N, C, expansion)) return ESMI_ERR_WORKSPACE;
    const int E = C * expansion;
    float* m1 = static_cast<float*>(workspace);
    float* m2 = reinterpret_cast<float*>(static_cast<char*>(workspace) + align256((size_t)B * N * E * 4));
    hipStream_t st = S(stream);
    if (int rc = launch_mixffn_front(B, N, C, E, x, {mlp1_w, nullptr}, mlp1_b, {conv_w, nullptr}, conv_b, m1, m2, st)) return rc;
    return launch_convgemm(linear(B, N, E, C, m2, E, {mlp2_w, nullptr}, mlp2_b, out, C), st);   // mlp2, blocks.py:28
}

int esmi_acoustic_decoder_f32(const esmi_predictor_weights* w, int dim, int B, int T, int duration, const float* x, int ldx,
                              float* pred, float* features, void* workspace, size_t workspace_bytes, esmi_stream_t stream) {
    if (!w || !x || !pred || !workspace || dim <= 0 || B <= 0 || T <= 0 || ldx < dim) return ESMI_ERR_ARG;
    if (duration && !features) return ESMI_ERR_ARG;
    if (workspace_bytes < esmi_variance_adaptor_workspace_bytes(B, T, dim)) return ESMI_ERR_WORKSPACE;
    return launch_predictor(w, dim, B, T, x, ldx, static_cast<float*>(workspace), pred, duration ? features : nullptr, dim, 0, nullptr, S(stream));
}

int esmi_bucket_embedding_f32(const float* v, const float* bins, const float* emb, int64_t rows, int dim, float* out,
                              int32_t* idx, esmi_stream_t stream) {
    if (!v || !bins || !emb || !out || rows <= 0 || dim <= 1) return ESMI_ERR_ARG;
    const long n = (long)rows * dim;
    ESMI_LAUNCH(bucket_embed_kernel, dim3(grid1d(n)), dim3(256), 0, S(stream), v, bins, emb, (long)rows, dim, out, idx);
    return launch_status();
}

int esmi_max_i32(const int32_t* v, int n, int32_t* out, esmi_stream_t stream) {
    if (!v || !out || n <= 0) return ESMI_ERR_ARG;
    ESMI_LAUNCH(max_i32_kernel, dim3(1), dim3(64), 0, S(stream), v, n, out);
    return launch_status();
}

int esmi_length_regulate_i32(const int32_t* dur, int B, int T, int32_t* cum, int32_t* mel_len, int32_t* lmax,
                             esmi_stream_t stream) {
    if (!dur || !cum || !mel_len || !lmax || B <= 0 || T <= 0) return ESMI_ERR_ARG;
    hipError_t e = hipMemsetAsync(lmax, 0, sizeof(int32_t), S(stream));
    if (e != hipSuccess) return (int)e;
    launch_length_regulate(dur, B, T, cum, mel_len, lmax, S(stream));
    return launch_status();
}

int esmi_length_regulator_indices_i32(const int32_t* cum, int B, int T, int L, int32_t* idx, esmi_stream_t stream) {
    if (!cum || !idx || B <= 0 || T <= 0 || L <= 0) return ESMI_ERR_ARG;
    const long n = (long)B * L;
    ESMI_LAUNCH(lr_indices_kernel, dim3(grid1d(n)), dim3(256), 0, S(stream), cum, B, T, L, idx);
    return launch_status();
}

int esmi_upsample_f32(const float* feat, const uint8_t* fmask, const int32_t* cum, int B, int T, int C, int L,
                      float* features, uint8_t* masks, esmi_stream_t stream) {
    if (!feat || !cum || !features || B <= 0 || T <= 0 || L <= 0 || (C & 3)) return ESMI_ERR_ARG;
    const long n = (long)B * L * (C / 4);
    ESMI_LAUNCH(upsample_kernel, dim3(grid1d(n)), dim3(256), 0, S(stream), feat, fmask, cum, B, T, C, L,
                features, masks);
    return launch_status();
}

int esmi_mask_rows_f32(float* x, const uint8_t* mask, int64_t rows, int C, esmi_stream_t stream) {
    if (!x || !mask || rows <= 0 || C <= 0) return ESMI_ERR_ARG;
    const long n = (long)rows * C;
    ESMI_LAUNCH(mask_rows_kernel, dim3(grid1d(n)), dim3(256), 0, S(stream), x, mask, (long)rows, C);
    return launch_status();
}

// ------------------------------------------------------------------ whole forward behind one call
namespace {
struct FwdArena {
    size_t feats[ESMI_MAX_DEPTH], ws, feat, preds[3], idx[2], dur, cum, h0, total;
    int n[ESMI_MAX_DEPTH];
};
int fwd_arena(const esmi_forward_args* a, FwdArena* o) {
    if (!a || a->depth < 1 || a->depth > ESMI_MAX_DEPTH || a->B <= 0 || a->T <= 0 || a->dim <= 0) return ESMI_ERR_ARG;
    size_t off = 0, ws = 0;
    int n_in = a->T;
    for (int i = 0; i < a->depth; ++i) {
        esmi_encoder_block_shape sh = a->shapes[i];
        sh.B = a->B; sh.n_in = n_in;
        const int n = conv_out_len(n_in, sh.kernel, sh.stride, sh.kernel / 2);
        if (n <= 0) return ESMI_ERR_ARG;
        o->n[i] = n;
        o->feats[i] = off; off += align256((size_t)a->B * n * sh.c_out * 4);
        const size_t w = esmi_encoder_block_workspace_bytes(&sh);
        ws = w > ws ? w : ws;
        n_in = n;
    }
    const size_t wv = esmi_fuse_variance_adaptor_workspace_bytes(a->B, a->T, a->dim, a->depth);
    ws = wv > ws ? wv : ws;
    const size_t rows = (size_t)a->B * a->T;
    o->ws = off; off += align256(ws);
    o->feat = off; off += align256(rows * 4 * a->dim * 4);
    for (int q = 0; q < 3; ++q) { o->preds[q] = off; off += align256(rows * 4); }
    for (int q = 0; q < 2; ++q) { o->idx[q] = off; off += align256(rows * 4); }
    o->dur = off; off += align256(rows * 4);
    o->cum = off; off += align256(rows * 4);
    o->h0 = off; off += (a->head.proj_wp || a->head.proj_w) ? align256(rows * a->head.dx2 * 4) : 0;
    o->total = off;
    return ESMI_OK;
}
}  // namespace

// The decoder re-uses the encoder side's scratch for its carried rows (dx2 = 256 chunk walk).  When that scratch is too small for a
// batch (few utterances, long output) the arena carries a tail region for them behind everything else -- the layout of the other
// regions never depends on L_out, so a stage-2 call with the length filled in later sees the same offsets.
static size_t fwd_dec_tail(const esmi_forward_args* a, const FwdArena& o) {
    // (L_out unknown at sizing time -- the reference's own call style: stage 1, host sync, stage 2 -- : the need of an arbitrarily long
    // output, which is bounded: the segmentation never uses more workgroups than max(B, one per CU).  Both call styles then run the same
    // decoder form)
    const size_t need = esmi_mel_decoder_workspace_bytes(&a->dec_shape, a->B, a->L_out > 0 ? a->L_out : -1);
    return need > o.feat - o.ws ? align256(need) : 0;
}
size_t esmi_forward_arena_bytes(const esmi_forward_args* a) {
    FwdArena o;
    return fwd_arena(a, &o) == ESMI_OK ? o.total + fwd_dec_tail(a, o) : 0;
}

static int forward_impl(const esmi_forward_args* a, const esmi_prosody_curves* ctl, int precision, int stage, esmi_stream_t stream);
int esmi_phoneme2mel_forward_f32(const esmi_forward_args* a, int stage, esmi_stream_t stream) {
    return esmi_phoneme2mel_forward_curve_f32(a, nullptr, 32, stage, stream);
}
int esmi_phoneme2mel_forward_ctl_f32(const esmi_forward_args* a, const esmi_prosody_control* ctl, int stage, esmi_stream_t stream) {
    return esmi_phoneme2mel_forward_curve_f32(a, PerUtterance(ctl).curves(), 32, stage, stream);
}
int esmi_phoneme2mel_forward_prec_f32(const esmi_forward_args* a, const esmi_prosody_control* ctl, int precision, int stage, esmi_stream_t stream) {
    return esmi_phoneme2mel_forward_curve_f32(a, PerUtterance(ctl).curves(), precision, stage, stream);
}
int esmi_phoneme2mel_forward_curve_f32(const esmi_forward_args* a, const esmi_prosody_curves* ctl, int precision, int stage, esmi_stream_t stream) {
    if (!a) return ESMI_ERR_ARG;
    // the precision argument of every form of this call is judged here, before the encoder side is enqueued
    if (stage == 1) precision = 32;   // (the encoder side has one arithmetic: stage 1 ignores the argument)
    PrecisionMode mode;
    if (int rc = precision_mode(precision, &mode)) return rc;
    if (!precision_mode_built(mode)) return ESMI_ERR_UNSUPPORTED;   // no one-product path in this build: refused before the encoder side is enqueued
    if (stage != 2 && ctl_conflict(ctl, nullptr, nullptr, a->dur_forced)) return ESMI_ERR_ARG;   // (a forced duration is final)
    if (!a->range_flag) return forward_impl(a, ctl, precision, stage, stream);
#if ESMI_RANGE_CHECK
    // validation mode: clear the word, point every translation unit's kernels at it, run, wait, read it back
    hipError_t e = hipMemsetAsync(a->range_flag, 0, sizeof(int32_t), S(stream));
    if (e != hipSuccess) return (int)e;
    for (const RangeSetter* u = g_range_setters; u; u = u->next)
        if (int rc = u->set(reinterpret_cast<int*>(a->range_flag))) return rc;
    int rc = forward_impl(a, ctl, precision, stage, stream);
    int32_t flag = 0;
    if (!rc) rc = read_device_flag(a->range_flag, S(stream), &flag);
    for (const RangeSetter* u = g_range_setters; u; u = u->next) u->set(nullptr);
    return rc ? rc : (flag ? ESMI_ERR_RANGE : ESMI_OK);
#else
    return ESMI_ERR_UNSUPPORTED;   // this library was built without the range check (libesmi_checked.so has it)
#endif
}
namespace {
// The encoder blocks' shapes of a one-call forward, the padding mask pooled to each block's length included: networks.py:69-70,
// pool = round(T / n), half to even; ESMI_ERR_UNSUPPORTED when that pool does not give back n.
int block_shapes(const esmi_forward_args* a, const FwdArena& o, int plan, esmi_encoder_block_shape* sh) {
    int n_in = a->T;
    for (int i = 0; i < a->depth; ++i) {
        sh[i] = a->shapes[i];
        sh[i].B = a->B; sh[i].n_in = n_in; sh[i].plan = plan; sh[i].mask_pool = 1; sh[i].mask_len = a->T;
        if (a->mask) {
            sh[i].mask_pool = (int)nearbyint((double)a->T / o.n[i]);
            if ((a->T + sh[i].mask_pool - 1) / sh[i].mask_pool != o.n[i]) return ESMI_ERR_UNSUPPORTED;
        }
        n_in = o.n[i];
    }
    return ESMI_OK;
}

// The whole encoder side as ONE launch (enc_all16_kernel: block 0 | block 1 | Fuse + variance adaptor + scan + head behind each other in
// one workgroup per utterance) when each of the three chain16 bodies serves its stage; ESMI_ERR_UNSUPPORTED otherwise.
int encoder_side_one_launch(const esmi_forward_args* a, const esmi_encoder_block_shape* sh, const VaArgs& va, Head head, float* x0, float* x1) {
    // (the chain16 bodies are built for MixFFN expansion 1 only, like launch_enc_block16)
    if (va.plan != ESMI_FUSE_ALL || a->depth != 2 || a->T > 128 || sh[0].expansion != 1 || sh[1].expansion != 1) return ESMI_ERR_UNSUPPORTED;
    const esmi_encoder_block_weights *w0 = &a->blocks[0], *w1 = &a->blocks[1];
    const bool want_head = a->head.proj_wp || a->head.proj_w;
    if (!block_packed(w0) || !w0->qk_wp || !w0->vo_wp || !block_packed(w1) || !w1->qk_wp || !w1->vo_wp || !va_chain_ok(va) ||
        (want_head && head != Head::in_chain) || !va.pw[0]->bins || !va.pw[0]->emb || !va.pw[1]->bins || !va.pw[1]->emb ||
        (va.n_i[1] - 1) * 2 + va.kernel < va.T)
        return ESMI_ERR_UNSUPPORTED;
    EncAttnFfnP b0 = block_params(w0, &sh[0], a->ids, a->embed, nullptr, va.mask, nullptr, nullptr, x0);
    EncAttnFfnP b1 = block_params(w1, &sh[1], nullptr, nullptr, x0, va.mask, nullptr, nullptr, x1);
    fold_attention(w0, &b0); fold_attention(w1, &b1);
    b0.wgs_per_b = b1.wgs_per_b = 1;
    int nw;
    FuseVaP p = va_chain_params(va, head == Head::in_chain, &nw);
    if (va.lean && head == Head::in_chain) drop_unread_outputs(&p);
    return p.cum ? launch_enc_all16(b0, b1, sh[1].c_in, p, va.dim, va.kernel, S(va.stream)) : ESMI_ERR_UNSUPPORTED;
}
}  // namespace

static int forward_impl(const esmi_forward_args* a, const esmi_prosody_curves* ctl, int precision, int stage, esmi_stream_t stream) {
    FwdArena o;
    int rc = fwd_arena(a, &o);
    if (rc) return rc;
    if (!a->ids || !a->mel_len || !a->duration_pred || !a->arena || stage < 0 || stage > 2) return ESMI_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(a->arena) & 15u) || a->arena_bytes < o.total) return ESMI_ERR_WORKSPACE;
    char* base = static_cast<char*>(a->arena);
    auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    auto I = [&](size_t off) { return reinterpret_cast<int32_t*>(base + off); };
    const int B = a->B, T = a->T, plan = a->plan & ESMI_FUSE_ALL;
    float* feat = F(o.feat);
    int32_t* cum = a->cum ? a->cum : I(o.cum);
    float* h0 = (a->head.proj_wp || a->head.proj_w) ? F(o.h0) : nullptr;
    const uint8_t* mask = a->mask;
    const float* feats[ESMI_MAX_DEPTH];
    for (int i = 0; i < a->depth; ++i) feats[i] = F(o.feats[i]);
    VaArgs va{&a->fuse, a->depth, a->dim, a->fuse_kernel, B, T, feats, o.n, {&a->pitch, &a->energy, &a->duration}, mask, nullptr, nullptr,
              a->dur_forced, feat,
              {a->pitch_pred ? a->pitch_pred : F(o.preds[0]), a->energy_pred ? a->energy_pred : F(o.preds[1]), a->duration_pred},
              a->pitch_idx ? a->pitch_idx : I(o.idx[0]), a->energy_idx ? a->energy_idx : I(o.idx[1]), a->dur ? a->dur : I(o.dur), cum,
              a->mel_len, nullptr, nullptr, plan, base + o.ws, esmi_fuse_variance_adaptor_workspace_bytes(B, T, a->dim, a->depth), stream,
              !a->pitch_pred && !a->energy_pred && !a->pitch_idx && !a->energy_idx,
              (ctl && stage != 2) ? *ctl : esmi_prosody_curves{}};   // (stage 2, the decoder alone, ignores the controls)
    // the decoder's first stage at phoneme rate: stage 1 produces h0, stage 2 reads it (a stage-2 call re-derives the same static test)
    const Head head = phoneme_rate_head(va, &a->head);
    const bool head_ok = head == Head::in_chain || (head == Head::gemm && a->head.dx2 == a->dec_shape.dx2);
    if (head_ok) { va.head = &a->head; va.h0 = h0; }
    if (stage != 2) {
        esmi_encoder_block_shape sh[ESMI_MAX_DEPTH];
        if ((rc = block_shapes(a, o, plan, sh))) return rc;
        rc = encoder_side_one_launch(a, sh, va, head, F(o.feats[0]), F(o.feats[1]));
        if (rc == ESMI_ERR_UNSUPPORTED) {   // block by block, then the Fuse + variance-adaptor stage
            rc = ESMI_OK;
            for (int i = 0; i < a->depth && !rc; ++i)
                rc = esmi_encoder_block_f32(&a->blocks[i], &sh[i], i == 0 ? a->ids : nullptr, i == 0 ? a->embed : nullptr,
                                            i == 0 ? nullptr : feats[i - 1], mask, F(o.feats[i]), base + o.ws,
                                            esmi_encoder_block_workspace_bytes(&sh[i]), stream);
            if (!rc) rc = fuse_variance_adaptor(va);
        }
        if (rc) return rc;
        if (a->lmax_dev && (rc = esmi_max_i32(a->mel_len, B, a->lmax_dev, stream))) return rc;
    }
    if (stage != 1) {
        if (a->L_out <= 0) return ESMI_OK;   // every duration zero: empty mel, nothing to launch
        if (!a->mel || !a->dec_blob) return ESMI_ERR_ARG;
        // the decoder's carried rows: the encoder side's scratch (free again), or the arena's tail region when that is too small
        const size_t dec_need = esmi_mel_decoder_workspace_bytes(&a->dec_shape, B, a->L_out);
        const bool use_tail = dec_need > o.feat - o.ws && a->arena_bytes >= o.total + dec_need;
        rc = esmi_mel_decoder_prec_f32(a->dec_blob, &a->dec_shape, feat, head_ok ? h0 : nullptr, cum, a->mel_len,
                                       a->lmax_host < 0 ? a->lmax_dev : nullptr, a->lmax_host, mask != nullptr && B > 1, B, T, a->L_out,
                                       a->mel, use_tail ? base + o.total : base + o.ws, use_tail ? a->arena_bytes - o.total : o.feat - o.ws,
                                       precision, stream);
        if (rc) return rc;
    }
    return ESMI_OK;
}

}  // extern "C"
