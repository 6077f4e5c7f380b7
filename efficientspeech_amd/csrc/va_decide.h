// The variance adaptor's discrete decisions (networks.py:349-384, 233-244), one definition each: which value is bucketized, how a
// duration is rounded, masked and clamped, what the length regulator's scan sums, the LDS edge count, and the workgroup scan.
// The kernels that decide -- enc_va16 (also enc_all16's tail), enc_va64, enc_pred128, enc_fuse_va, va_tail -- call these; which
// kernel still spells which piece out (enc_fuse_va: the bucket input and the duration, on va_row_scale's scale), and why (its listing against the parent's), is in profiles/va_decide_refactor.md.
// Only __device__ __forceinline__ functions on values the caller already holds.
#pragma once
#include "esmi_dev.h"

namespace esmi {

// bits of the parameter structs' `curve` field (FuseVaP, Pred128P, VaTailP): the quantity's teacher pointer holds a (B, T) prosody curve
constexpr int kCurvePitch = 1, kCurveEnergy = 2, kCurveDur = 4;

// the value torch.bucketize sees: the teacher value on a row that has one, else the prediction times the utterance's prosody scale
// (a teacher value is never scaled)
__device__ __forceinline__ float va_bucket_input(bool teacher_row, float teacher, float pred, float scale) {
    return teacher_row ? teacher : pred * scale;
}

// the scale of a row's prediction: the utterance's (B) control, or -- `curve`, a wave-uniform bit of the parameter struct's `curve`
// field -- the row's own entry of a (B, T) curve.  The curve's entry arrives in the row's teacher-value slot (the host points the
// teacher resource at the curve: the two are mutually exclusive, so a curve costs no load of its own).  A padding row and a row past
// the utterance's end take 1: whatever the curve holds there (NaN, 1e30) is never used.
__device__ __forceinline__ float va_row_scale(bool curve, float row_val, float utt_scale, bool pad_or_out) {
    return curve ? (pad_or_out ? 1.0f : row_val) : utt_scale;
}

// the fp32 duration that is stored as (int)dval: the forced duration, else torch.round (half to even) of the scaled prediction;
// under a mask a padding row gives 0 and nothing is negative (networks.py:381-382)
__device__ __forceinline__ float va_duration(bool forced, float forced_val, float pred, float scale, bool has_mask, bool pad) {
    float d = forced ? forced_val : rintf(pred * scale);
    if (has_mask) {
        if (pad) d = 0.0f;
        d = fmaxf(d, 0.0f);
    }
    return d;
}

// what FeatureUpsampler's scan sums for the row (`.int()`, networks.py:234, then max(., 0)); a row past the utterance's end adds nothing
__device__ __forceinline__ int va_scan_term(float dval, bool out_of_range) {
    return out_of_range ? 0 : max((int)dval, 0);
}

// torch.bucketize(v, edges, right=False) = the number of edges strictly below v: this lane's share over N4 float4 of LDS, as an fp32
// count (sums of 0 / 1: exact in any order); the caller's row_sum4 adds the four lanes of the row.
// NaN: `e < NaN` is false for every edge, so a NaN value gets bucket 0 -- here, in enc_fuse_va's register-resident edges, in
// bucketize_left (va_tail, bucket_embed_kernel) and in the C oracle alike.  torch.bucketize sorts NaN above everything and answers
// dim - 1.  Either index is inside the embedding table; the project's rule is 0 and tests/test_va_ties.py pins it.
template <int N4>
__device__ __forceinline__ float bucket_count_lds(const float* edges, float v) {
    float cnt = 0.0f;
#pragma unroll
    for (int k4 = 0; k4 < N4; ++k4) {
        const f32x4 e0 = ld4(edges + 4 * k4);
#pragma unroll
        for (int e = 0; e < 4; ++e) cnt += e0[e] < v ? 1.0f : 0.0f;
    }
    return cnt;
}

// FeatureUpsampler's scan (networks.py:233-244) while the durations are still on the CU: cum_b[0 .. T) = inclusive cumsum of the
// scan terms sdur[0 .. T) (LDS), *mel_len_b = its total.  ONE wave of the workgroup calls it (all 64 lanes), behind the caller's
// own barrier that publishes sdur; lane l takes the ceil(T / 64) positions from l * ceil(T / 64).
// Positions >= T (the last lanes' tails, lanes with no position at all) are not selected away: their byte offset (>= 4 T) falls off
// the end of the T * 4-byte buffer resource.  That offset travels in buf_st_i's VECTOR offset, which the hardware range-checks
// against the resource's size per lane, so the store is dropped and the words behind cum_b's row are never written.
__device__ __forceinline__ void wg_scan_durations(const int* sdur, int T, int* cum_b, int* mel_len_b, int lane) {
    const int per = (T + 63) / 64, q0 = lane * per;
    int local = 0;
    for (int q = 0; q < per; ++q) local += (q0 + q < T) ? sdur[q0 + q] : 0;
    int incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = shfl_up_i(incl, d);
        if (lane >= d) incl += v;
    }
    const BufRsrc r_cum = make_rsrc(cum_b, (long)T * 4);
    int run = incl - local;
    for (int q = 0; q < per; ++q) {
        run += (q0 + q < T) ? sdur[q0 + q] : 0;
        buf_st_i(r_cum, (unsigned)((q0 + q) * 4), run);
    }
    const int total = shfl_i(incl, 63);
    if (lane == 0) *mel_len_b = total;
}

}  // namespace esmi
