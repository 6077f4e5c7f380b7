// Parameter structs of the Fuse + variance-adaptor kernels (enc_fuse_va.h, enc_va16.h, enc_va64.h, enc_fuse128.h, enc_pred128.h) and of
// the register-resident encoder-block kernels (enc_ffn64.h, enc_ffn128.h, enc_merge256.h): what the launchers (launch.h) take.
#pragma once

namespace esmi {

struct PredW {   // conv1_w / conv2_w in MFMA B-fragment order (esmi_pack_bfrag_f32)
    const float *conv1_w, *conv1_b, *ln1_g, *ln1_b, *conv2_w, *conv2_b, *ln2_g, *ln2_b, *lin_w, *lin_b, *bins, *emb;
};

// enc_pred128.h (dim = 128: one workgroup per (utterance, predictor))
struct Pred128P {
    PredW pred[3];                  // conv1_w / conv2_w: esmi_pack_bfrag_f32 arrays (three taps each)
    const unsigned char* mask;      // (B, T) or NULL
    const float* pitch_t;           // teacher values (train = True) or NULL
    const float* energy_t;
    const int* dur_t;
    float* feat;                    // (B, T, 4 dim): channels [0, dim) are read, the rest written
    float* preds[3];                // (B, T) each
    int* pitch_idx;
    int* energy_idx;
    int* dur;
    int* cum;                       // (B, T) or NULL
    int* mel_len;                   // (B)
    int B, T;
    const float *pitch_s, *energy_s, *dur_s;   // prosody controls: (B) scale of the prediction that is bucketized / rounded, or NULL = 1
    int curve;                      // kCurve* bits: that quantity's teacher pointer above holds a (B, T) fp32 prosody curve instead (FuseVaP::curve)
};
// enc_ffn64.h (everything behind the attention of a C = 64, one-head block: one workgroup per utterance)
struct PostAttn64P {
    const float* ctx;        // (B, N, 64) attention context
    const float* x;          // (B, N, 64) the block's input rows (residual)
    float* out;              // (B, N, 64)
    const float *proj_w, *ffn_w, *mlp2_w;   // esmi_pack_bfrag_f32 arrays (ffn_w: three taps)
    const float *proj_b, *ln1_g, *ln1_b, *ffn_b, *ffn_b0, *ffn_b2, *mlp2_b, *ln2_g, *ln2_b;
    const unsigned char* rowmask;            // (B, N) 1 = padding row, or NULL
    int B, N;
};
// enc_ffn128.h (everything behind the attention of a C = 128, two-head, expansion-2 block: one workgroup per utterance)
struct PostAttn128P {
    const float* ctx;        // (B, N, 256) attention context (two heads x 128)
    const float* x;          // (B, N, 128) the block's input rows (residual)
    float* y1;               // (B, N, 128) scratch: LN1's output (the second residual)
    float* out;              // (B, N, 128); may be x
    const float *proj_w, *ffn_w, *mlp2_w;   // esmi_pack_bfrag_f32 arrays: (128 x 256), three taps of (256 x 128), (128 x 256)
    const float *proj_b, *ln1_g, *ln1_b, *ffn_b, *ffn_b0, *ffn_b2, *mlp2_b, *ln2_g, *ln2_b;
    const unsigned char* rowmask;            // (B, N) 1 = padding row, or NULL
    int B, N;
};
// enc_merge256.h (merge convolution stride 2, 128 -> 256, + the folded attention's query GEMM 256 -> heads x 256: one workgroup per utterance)
struct MergeQ256P {
    const float* x_in;       // (B, n_in, 128)
    float* x_out;            // (B, n_out, 256)
    float* q;                // (B, n_out, heads * 256)
    const float *merge_w, *q_w;   // esmi_pack_bfrag_f32 arrays: `kernel` taps of (256 x 128); (heads * 256 x 256)
    int B, n_in, n_out, kernel, heads;
};
struct FuseVaP {
    int B, T, depth, kernel;
    const float* feats[4];
    int n_i[4];
    const float* mlp_w[4];  // mlp_w, up_w, fuse_w: MFMA B-fragment order (esmi_pack_bfrag_f32, see wave_chain.h)
    const float* mlp_b[4];
    const float* up_w[4];   // (k, dim, dim) tap-major
    const float* up_b[4];
    const float* fuse_w;    // (dim, depth*dim)
    const float* fuse_b;
    PredW pred[3];          // pitch, energy, duration
    const unsigned char* mask;
    const float* pitch_t;
    const float* energy_t;
    const int* dur_t;
    float* feat;            // (B,T,4*dim)
    float* preds[3];        // (B,T) each
    int* pitch_idx;
    int* energy_idx;
    int* dur;
    // optional decoder head, dim == 32 only (4*dim = dx2 = 128): h0 = LN(tanh(Linear(4*dim, dx2)(feat))) at phoneme rate
    const float *head_w, *head_b, *head_g, *head_beta;   // head_w in MFMA B-fragment order
    float* h0;              // (B,T,128) or NULL
    int* cum;               // (B,T) inclusive cumsum of max(dur,0) and
    int* mel_len;           // (B) its total: written when one workgroup covers the utterance (halo == 0), else NULL
    int wgs_per_b;          // workgroups per utterance
    int useful;             // positions stored per workgroup: 32*nw - 2*halo
    int halo;               // 0: one workgroup covers the sequence, 2: two recomputed rows per side
    // prosody controls (inference): (B) fp32 each or NULL = 1.  The value that is bucketized is pred * pitch_s[b] / pred * energy_s[b], the
    // duration rounds pred * dur_s[b]; one fp32 multiply each (va_decide.h).  Teacher / forced values are never scaled, preds[] stay the raw predictions.
    const float *pitch_s, *energy_s, *dur_s;
    // per-phoneme prosody curves: bit q set (kCurvePitch / kCurveEnergy / kCurveDur) = pitch_t / energy_t / dur_t does not hold teacher
    // values but a (B, T) fp32 curve, the scale of each row's own prediction (va_decide.h: va_row_scale); that quantity's *_s is NULL then.
    // A runtime field, wave-uniform: the kernels keep one instantiation and the row's one teacher-slot load serves either meaning.
    int curve;
};

}  // namespace esmi
