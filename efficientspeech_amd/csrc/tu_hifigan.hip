// esmi C-ABI, translation unit "tu_hifigan.hip": the HiFi-GAN generator -- the one-launch ResBlock kernels and their weight packer
// (hifigan_resblock.h) and the generator's host side (esmi_hifigan_*; its convolutions run on tu_convgemm.hip's kernels)
// One of several translation units of libesmi.so (compiled in parallel by __graft_entry__.build(); the simulator build
// tools/wavesim/build.sh compiles the same files with the host compiler).  Internal launchers are declared in launch.h.
#include "launch.h"

using namespace esmi;
ESMI_TU_RANGE_SETTER(hifigan)

ESMI_RESBLOCK_INSTANCE(PM_SPLIT)   // the fp32-accurate ResBlock kernels (launch.h has the ladder)

// ------------------------------------------------------------------ the generator's host side
namespace {
// checks the generator's shape; *buf: bytes of one activation buffer (the largest B * N * C of the chain)
int hg_plan(const esmi_hifigan_shape* s, int B, int L, size_t* buf) {
    if (!s || B <= 0 || L <= 0 || s->n_up < 1 || s->n_up > ESMI_HIFIGAN_MAX_UP || s->n_kernels < 1 ||
        s->n_kernels > ESMI_HIFIGAN_MAX_KERNELS || (s->resblock != 1 && s->resblock != 2) || s->n_mel <= 0 || (s->n_mel & 7))
        return ESMI_ERR_ARG;
    if (s->n_up * s->n_kernels * 3 > ESMI_HIFIGAN_MAX_RBCONV) return ESMI_ERR_UNSUPPORTED;
    long n = L;
    int c = s->initial_channel;
    size_t mx = (size_t)B * n * c;
    for (int i = 0; i < s->n_up; ++i) {
        if (s->up_rates[i] < 1 || s->up_kernels[i] < s->up_rates[i] || ((s->up_kernels[i] - s->up_rates[i]) & 1) || (c & 15)) return ESMI_ERR_UNSUPPORTED;
        n *= s->up_rates[i];
        c /= 2;
        const size_t e = (size_t)B * n * c;
        mx = e > mx ? e : mx;
    }
    if (c & 7) return ESMI_ERR_UNSUPPORTED;   // implicit-GEMM k-steps are 8 channels
    *buf = align256(mx * 4);
    return ESMI_OK;
}

// one-sided receptive field of ResBlock j of a stage: sum((k - 1) / 2 . dilation) over its convolutions
int rb_halo(const esmi_hifigan_shape* s, int j) {
    const int nconv = s->resblock == 1 ? 3 : 2, half = (s->rb_kernels[j] - 1) / 2;
    int halo = 0;
    for (int m = 0; m < nconv; ++m) halo += half * s->rb_dilations[j * 3 + m] + (s->resblock == 1 ? half : 0);
    return halo;
}
// Length-aware call: how far behind an utterance's last mel frame each stage still has to be right for every KEPT sample (t < len . hop)
// to come out as in the full run -- the one-sided receptive field from that stage to the waveform, walked backwards: conv_post reads 3
// positions ahead; the ResBlocks of a stage the largest halo among them (one margin per stage: out (+)= block(x) then accumulates
// over the same rows for every block); ConvTranspose1d(k, u, pad (k - u) / 2) output t reads inputs up to floor((t + pad) / u), so m
// positions behind len . rate need ceil((m + pad) / u) behind len . rate / u; conv_pre reads 3 frames ahead.  Stage i (the output of
// ups[i] and its ResBlocks) then covers n_eff = min(n, len . mul[i] + add[i]) positions.
// hifigan.ragged_margins (Python; tools/bench_vocoder.py's ideal ratio) is the same walk written a second time: keep the two in step.
// This copy is bound by tests/test_vocoder_ragged.py on the device -- too short fails the bit-for-bit test on NaN-filled workspaces, and
// the margin test overwrites the mel from the frames the PYTHON copy claims on -- for v1 / v2 / v3; other shapes have no such test.
struct HgMargins { int mul[ESMI_HIFIGAN_MAX_UP], add[ESMI_HIFIGAN_MAX_UP]; };
HgMargins hg_margins(const esmi_hifigan_shape* s) {
    HgMargins g = {};
    int rate = 1, need = 3;
    for (int i = 0; i < s->n_up; ++i) g.mul[i] = rate *= s->up_rates[i];
    for (int i = s->n_up - 1; i >= 0; --i) {
        int halo = 0;
        for (int j = 0; j < s->n_kernels; ++j) halo = rb_halo(s, j) > halo ? rb_halo(s, j) : halo;
        g.add[i] = need + halo;
        const int u = s->up_rates[i], pad = (s->up_kernels[i] - u) / 2;
        need = (g.add[i] + pad + u - 1) / u;
    }
    return g;
}

// mode: precision 16 and bf16 have the window of the one-product kernels -- half the LDS per row, and 16 waves at 64 channels (rb_amp_rmax)
bool resblock_fused_ok(const esmi_hifigan_weights* w, const esmi_hifigan_shape* s, int rb, int c, int k, int n, PrecisionMode mode, ResblockP* o) {
#if !ESMI_CHAIN_SPLIT
    return false;   // the exact-fp32 build keeps the per-conv fp32-MFMA launches
#endif
    if ((c != 8 && c != 16 && c != 32 && c != 64) || (k != 3 && k != 7 && k != 11)) return false;   // the instantiations
    const int nconv = s->resblock == 1 ? 3 : 2, j = rb % s->n_kernels;
    ResblockP p = {};
    const int halo = rb_halo(s, j);
    int q = 0;
    for (int m = 0; m < nconv; ++m) {
        const int d = s->rb_dilations[j * 3 + m];
        if (d < 1 || !w->rb_wp1[rb * 3 + m] || !w->rb_b1[rb * 3 + m]) return false;
        p.conv[q++] = RbConv{static_cast<const unsigned*>(w->rb_wp1[rb * 3 + m]), w->rb_b1[rb * 3 + m], d, s->resblock == 1 ? 0 : 1};
        if (s->resblock == 1) {
            if (!w->rb_wp2[rb * 3 + m] || !w->rb_b2[rb * 3 + m]) return false;
            p.conv[q++] = RbConv{static_cast<const unsigned*>(w->rb_wp2[rb * 3 + m]), w->rb_b2[rb * 3 + m], 1, 1};
        }
    }
    // 8 waves = 8 (row pair, 32-channel tile) items; LDS <= 80 KB: two workgroups per CU
    const int r_max = mode != PM_SPLIT ? rb_amp_rmax(c) : (c == 64 ? 256 : 512);
    int R = ((n + 2 * halo + 63) / 64) * 64;
    R = R < r_max ? R : r_max;
    if (R - 2 * halo < 32 && R - 2 * halo < n) return false;
    p.n_conv = q; p.k = k; p.halo = halo; p.R = R; p.TL = R - 2 * halo; p.n = n;
    p.tiles_per_b = (n + p.TL - 1) / p.TL;
    *o = p;
    return true;
}

constexpr float kSlope = 0.1f;   // LRELU_SLOPE, hifigan/models.py:17

// One stage of the generator (the output of ups[i] and its ResBlocks) as its launches see it: n positions per utterance on c channels,
// and in a length-aware call, from the first stage of at most 64 channels on, the stage's limit n_eff = min(n, len . mul + add)
struct HgStage {
    int B, n, c;
    const int32_t* len;   // mel frames per utterance (device memory); nullptr: not limited
    int len_max, len_mul, len_add;
    template <class P>    // ConvGemmP and ResblockP carry the same four fields
    void limit(P* p) const { if (len) { p->len = len; p->len_max = len_max; p->len_mul = len_mul; p->len_add = len_add; } }
};

// ResBlock rb of stage g one launch per convolution: x (+)= block(y), j = rb % n_kernels > 0 accumulates; r, t: the block's own state
int resblock_conv_by_conv(const esmi_hifigan_weights* w, const esmi_hifigan_shape* s, const HgStage& g, int rb, const float* y, float* x,
                          float* r, float* t, PrecisionMode mode, hipStream_t st) {
    const int j = rb % s->n_kernels, k = s->rb_kernels[j], nconv = s->resblock == 1 ? 3 : 2, c = g.c;
    auto conv = [&](int dil, const float* in, const float* wt, const float* bias, float* out) {   // out = conv(leaky_relu(in))
        ConvGemmP p = conv1d(g.B, g.n, c, c, k, dil, in, c, {wt, nullptr}, bias, out, c);
        p.act_in = 1; p.act_in_slope = kSlope; p.amp = mode;
        g.limit(&p);
        return p;
    };
    const float* cur = y;                   // the ResBlock's running x (first iteration: the stage input itself)
    for (int m = 0; m < nconv; ++m) {
        const int d = s->rb_dilations[j * 3 + m], i = rb * 3 + m;
        const bool last = m + 1 == nconv;   // last iteration: straight into the stage sum (accumulated for j > 0)
        ConvGemmP p;
        float* dst;
        if (s->resblock == 1) {
            // xt = c1(leaky_relu(x)); xt = c2(leaky_relu(xt)); x = xt + x   (models.py:49-54)
            // buffers: cur in {y, r}; c1 writes t; c2 reads t, adds cur, writes dst in {r (in place when cur == r), x}
            if (int rc = launch_convgemm(conv(d, cur, w->rb_w1[i], w->rb_b1[i], t), st)) return rc;
            dst = last ? x : r;
            p = conv(1, t, w->rb_w2[i], w->rb_b2[i], dst);
        } else {
            // xt = c(leaky_relu(x)); x = xt + x   (models.py:75-79): the conv reads neighbours of x, so not in place
            dst = last ? x : (cur == r ? t : r);
            p = conv(d, cur, w->rb_w1[i], w->rb_b1[i], dst);
        }
        p.res = cur; p.ldr = c; p.accum = last && j > 0;
        if (int rc = launch_convgemm(p, st)) return rc;
        cur = dst;
    }
    return ESMI_OK;
}

// Every weight the call is going to read, looked at before the first launch: conv_pre, conv_post and the ConvTranspose1d's their fp32
// tensor and bias; a ResBlock that runs as one launch (fp[rb].n_conv > 0 then, and fp[rb] holds its parameters) its packed weights
// and biases (resblock_fused_ok has looked), any other its fp32 tensors and biases.
bool hg_weights_ok(const esmi_hifigan_weights* w, const esmi_hifigan_shape* s, int L, PrecisionMode mode, ResblockP* fp) {
    bool ok = w->pre_w && w->pre_b && w->post_w && w->post_b;
    int n = L, c = s->initial_channel;
    for (int i = 0, rb = 0; i < s->n_up; ++i) {
        ok = ok && w->up_w[i] && w->up_b[i];
        n *= s->up_rates[i]; c /= 2;
        for (int j = 0; j < s->n_kernels; ++j, ++rb) {
            if (resblock_fused_ok(w, s, rb, c, s->rb_kernels[j], n, mode, &fp[rb])) continue;
            fp[rb].n_conv = 0;
            for (int m = rb * 3; m < rb * 3 + (s->resblock == 1 ? 3 : 2); ++m)
                ok = ok && w->rb_w1[m] && w->rb_b1[m] && (s->resblock == 2 || (w->rb_w2[m] && w->rb_b2[m]));
        }
    }
    return ok;
}

// The generator behind both entry points.  mel_len == nullptr: the plain call.  Otherwise (include/esmi.h) conv_pre and the stages of
// more than 64 channels compute every frame -- their convolutions run on the kernels that tile flat rows across utterances --, and from
// the first stage of at most 64 channels on every launch (ConvTranspose1d, the ResBlocks fused or conv by conv, conv_post) carries the
// stage's limit from hg_margins: a limited stage reads only rows the stage before it wrote, full or limited.  What that leaves
// unlimited, by multiply-adds (n . c^2 per stage): v2 (64 / 32 / 16 / 8 channels) conv_pre alone, a few per cent; v3 its 128-channel
// stage, about a fifth; v1 its 256- and 128-channel stages, about two thirds -- on v1 most of the padded work is still done.
// precision 0 / 32: the fp32-accurate split products.  16 (include/esmi.h): conv_pre, every ConvTranspose1d and every ResBlock convolution
// carry ConvGemmP::amp, a one-launch ResBlock runs on hifigan_resblock_amp_kernel / hifigan_resblock16_amp_kernel; conv_post is unchanged.
// ESMI_PRECISION_BF16: the same launches with ConvGemmP::amp = 2 (bfloat16 operands, nothing scaled) and the ResBlocks' bf16 kernels
// (hifigan_resblock_bf16_kernel / hifigan_resblock16_bf16_kernel: same window, same packed weights).
int hifigan_generator(const esmi_hifigan_weights* w, const esmi_hifigan_shape* s, const float* mel, int B, int L,
                      const int32_t* mel_len, float* wav, int16_t* pcm, int precision, void* workspace, size_t workspace_bytes,
                      esmi_stream_t stream) {
    PrecisionMode mode;   // which ResBlock kernels, and ConvGemmP::amp of the per-convolution launches
    if (int rc = precision_mode(precision, &mode)) return rc;
    size_t buf;
    int rc = hg_plan(s, B, L, &buf);
    if (rc) return rc;
    if (!precision_mode_built(mode)) return ESMI_ERR_UNSUPPORTED;   // the exact-fp32 build has no one-product path
    if (!w || !mel || (!wav && !pcm) || !workspace) return ESMI_ERR_ARG;
    if (workspace_bytes < 4 * buf) return ESMI_ERR_WORKSPACE;
    ResblockP fused[ESMI_HIFIGAN_MAX_RBCONV / 3];   // (hg_plan: n_up . n_kernels fit)
    if (!hg_weights_ok(w, s, L, mode, fused)) return ESMI_ERR_ARG;
    const HgMargins mg = hg_margins(s);
    static constexpr decltype(&launch_resblock<PM_SPLIT>) kLaunchResblock[kPrecisionModes] = {launch_resblock<PM_SPLIT>, launch_resblock<PM_F16>,
                                                                                              launch_resblock<PM_BF16>};
    hipStream_t st = S(stream);
    auto ws = [&](int q) { return reinterpret_cast<float*>(static_cast<char*>(workspace) + q * buf); };
    float *x = ws(0), *y = ws(1), *r = ws(2), *t = ws(3);   // x: stage input / sum over the ResBlocks; y: upsampled; r, t: ResBlock state
    HgStage g = {B, L, s->initial_channel, nullptr, 0, 0, 0};
    // conv_pre, models.py:112: Conv1d(n_mel, C0, 7, padding 3)
    ConvGemmP p = conv1d(B, L, s->n_mel, g.c, 7, 1, mel, s->n_mel, {w->pre_w, nullptr}, w->pre_b, x, g.c);
    p.amp = mode;
    if ((rc = launch_convgemm(p, st))) return rc;
    float in_scale = 1.0f;           // the mean over the ResBlocks of the previous stage, folded into the next input activation
    for (int i = 0; i < s->n_up; ++i) {
        const int u = s->up_rates[i], k = s->up_kernels[i];
        const HgStage in = g;
        const bool lim = mel_len && in.c / 2 <= 64;   // this stage runs under the per-utterance limit (and so does every later one)
        g = HgStage{B, in.n * u, in.c / 2, lim ? mel_len : nullptr, L, mg.mul[i], mg.add[i]};
        // x = ups[i](leaky_relu(x, 0.1)), models.py:114-115: ConvTranspose1d(c, c/2, k, u, padding (k-u)//2)
        p = conv_transpose1d(B, in.n, g.n, in.c, g.c, k, u, (k - u) / 2, x, in.c, {w->up_w[i], nullptr}, w->up_b[i], y, g.c);
        p.act_in = 1; p.act_in_slope = kSlope; p.a_scale = in_scale; p.amp = mode;
        g.limit(&p);
        if ((rc = launch_convgemm(p, st))) return rc;
        for (int j = 0; j < s->n_kernels; ++j) {   // xs += resblocks[i*num_kernels + j](x), models.py:116-121
            const int rb = i * s->n_kernels + j;
            ResblockP& fp = fused[rb];
            if (fp.n_conv) {   // the whole block on an LDS-resident window: y -> x (+)=
                fp.x = y; fp.out = x; fp.B = B; fp.accum = j > 0; fp.slope = kSlope;
                g.limit(&fp);
                rc = kLaunchResblock[mode](fp, g.c, st);
            } else {
                rc = resblock_conv_by_conv(w, s, g, rb, y, x, r, t, mode, st);
            }
            if (rc) return rc;
        }
        in_scale = 1.0f / (float)s->n_kernels;   // x = xs / num_kernels (models.py:122), applied where x is read next
    }
    // x = tanh(conv_post(leaky_relu(x))), models.py:123-125 (F.leaky_relu default slope 0.01)
    p = conv1d(B, g.n, g.c, 1, 7, 1, x, g.c, {w->post_w, nullptr}, w->post_b, wav, 1);
    p.act = ACT_TANH; p.act_in = 1; p.act_in_slope = 0.01f; p.a_scale = in_scale;
    if (!mel_len) return launch_convgemm(p, st);
    // every sample is written: the utterance's own, then exact zeros from len . hop on (no margin: these are the kept samples themselves)
    p.len = mel_len; p.len_max = L; p.len_mul = g.n / L; p.len_add = 0;
    return launch_conv_to1_len(p, pcm, st);
}
}  // namespace

extern "C" {

size_t esmi_hifigan_workspace_bytes(const esmi_hifigan_shape* s, int B, int L) {
    size_t buf;
    return hg_plan(s, B, L, &buf) == ESMI_OK ? 4 * buf : 0;
}

int esmi_hifigan_generator_f32(const esmi_hifigan_weights* w, const esmi_hifigan_shape* s, const float* mel, int B, int L,
                               float* wav, void* workspace, size_t workspace_bytes, esmi_stream_t stream) {
    return hifigan_generator(w, s, mel, B, L, nullptr, wav, nullptr, 32, workspace, workspace_bytes, stream);
}

int esmi_hifigan_generator_ragged_f32(const esmi_hifigan_weights* w, const esmi_hifigan_shape* s, const float* mel, int B, int L,
                                      const int32_t* mel_len, float* wav, int16_t* pcm, void* workspace, size_t workspace_bytes,
                                      esmi_stream_t stream) {
    if (!mel_len) return ESMI_ERR_ARG;
    return hifigan_generator(w, s, mel, B, L, mel_len, wav, pcm, 32, workspace, workspace_bytes, stream);
}

int esmi_hifigan_generator_prec_f32(const esmi_hifigan_weights* w, const esmi_hifigan_shape* s, const float* mel, int B, int L,
                                    const int32_t* mel_len, float* wav, int16_t* pcm, int precision, void* workspace,
                                    size_t workspace_bytes, esmi_stream_t stream) {
    if (!mel_len && pcm) return ESMI_ERR_ARG;   // the plain call has no PCM plane
    return hifigan_generator(w, s, mel, B, L, mel_len, wav, pcm, precision, workspace, workspace_bytes, stream);
}

size_t esmi_pack_resblock_bytes(int c, int k) {
    if ((c != 8 && c != 16 && c != 32 && c != 64) || (k != 3 && k != 7 && k != 11)) return 0;
    return rb_pack_dwords(c, k) * 4;
}
int esmi_pack_resblock_f16(const float* src, void* dst, int c, int k, esmi_stream_t stream) {
    if (!src || !dst) return ESMI_ERR_ARG;
    if (!esmi_pack_resblock_bytes(c, k)) return ESMI_ERR_UNSUPPORTED;
    if (c <= 16) {
        const long n16 = (long)rb_ksteps16(c, k) * 64;
        ESMI_LAUNCH(pack_resblock16_kernel, dim3(grid1d(n16)), dim3(256), 0, S(stream), src, static_cast<unsigned*>(dst), c, k);
        return launch_status();
    }
    const long n = (long)rb_mtiles(c) * rb_ksteps(c, k) * 64;
    ESMI_LAUNCH(pack_resblock_kernel, dim3(grid1d(n)), dim3(256), 0, S(stream), src, static_cast<unsigned*>(dst), c, k);
    return launch_status();
}

}  // extern "C"
