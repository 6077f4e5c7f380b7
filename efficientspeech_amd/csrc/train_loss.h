// Training step: the loss of model.py:167-216 and its gradient seeds, in two deterministic stages: kLossBlocks workgroups write partial
// sums (counts, mel |d|, three squared errors) in a fixed order, one workgroup adds them up; the gradient kernel then scales.
//   out[0..3] = mel L1, pitch MSE, energy MSE, log-duration MSE (means over the unmasked elements); out[4] = 10 a + 2 b + 2 c + d
#pragma once
#include "train_reduce.h"

namespace esmi {

struct LossP {
    const float *mel_pred, *mel, *pitch_pred, *pitch, *energy_pred, *energy, *dur_pred;
    const int* dur;
    const unsigned char *mel_mask, *ph_mask;   // 1 = padding; NULL = nothing masked
    int B, T, L, n_mel;
    float *out, *d_mel, *d_pitch, *d_energy, *d_dur;
    float* partial;                            // [kLossBlocks][6]
    const float* grad_seed;                    // NULL or one float: multiplies every gradient
};
// (kLossBlocks: wavesim_shim.h)
static __global__ __launch_bounds__(256) void train_loss_partial_kernel(const LossP p) {
    ESMI_DYN_LDS(red);   // 256 floats
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)kLossBlocks * 256;
    const long nf = (long)p.B * p.L, np_ = (long)p.B * p.T;
    float cnt_f = 0.0f, cnt_p = 0.0f, a = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (long r = tid; r < nf; r += nth) cnt_f += (p.mel_mask && p.mel_mask[r]) ? 0.0f : 1.0f;
    const int nm4 = p.n_mel >> 2;
    const long n4 = nf * nm4;
    if ((p.n_mel & 3) == 0 && n4 < 0x7FFFFFFFL && ((reinterpret_cast<uintptr_t>(p.mel_pred) | reinterpret_cast<uintptr_t>(p.mel)) & 15) == 0) {
        // 16 bytes per load, four (prediction, target) pairs in flight per thread, every load unconditional (a clamped index, the
        // surplus masked): the scalar form below ran 94 dependent element loads and as many 64-bit divisions per thread (81 us at
        // B = 128 for 49 MB)
        for (long q0 = tid; q0 < n4; q0 += 4 * nth) {
            f32x4 pv[4], tv[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long qq = q0 + u * nth;
                const unsigned qc = (unsigned)(qq < n4 ? qq : n4 - 1);
                ok[u] = qq < n4 && !(p.mel_mask && p.mel_mask[qc / (unsigned)nm4]);
                pv[u] = ld4(p.mel_pred + (long)qc * 4);
                tv[u] = ld4(p.mel + (long)qc * 4);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!ok[u]) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) a += fabsf(pv[u][e] - tv[u][e]);
            }
        }
    } else {
        for (long q = tid; q < nf * p.n_mel; q += nth)
            if (!(p.mel_mask && p.mel_mask[q / p.n_mel])) a += fabsf(p.mel_pred[q] - p.mel[q]);
    }
    for (long r = tid; r < np_; r += nth) {
        if (p.ph_mask && p.ph_mask[r]) continue;
        const float d1 = p.pitch_pred[r] - p.pitch[r], d2 = p.energy_pred[r] - p.energy[r];
        const float d3 = logf(p.dur_pred[r] + 1.0f) - logf((float)p.dur[r] + 1.0f);
        cnt_p += 1.0f; s1 = fmaf(d1, d1, s1); s2 = fmaf(d2, d2, s2); s3 = fmaf(d3, d3, s3);
    }
    const float v[6] = {cnt_f, cnt_p, a, s1, s2, s3};
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const float t = block_sum_256(v[e], red);
        if (threadIdx.x == 0) p.partial[(long)blockIdx.x * 6 + e] = t;
    }
}
static __global__ __launch_bounds__(256) void train_loss_final_kernel(const LossP p) {
    ESMI_DYN_LDS(red);
    float t[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) t[e] = block_sum_256((int)threadIdx.x < kLossBlocks ? p.partial[(long)threadIdx.x * 6 + e] : 0.0f, red);
    if (threadIdx.x == 0) {
        const float n_el = t[0] * (float)p.n_mel, n_ph = t[1];
        const float mel_l = t[2] / n_el, l1 = t[3] / n_ph, l2 = t[4] / n_ph, l3 = t[5] / n_ph;
        p.out[0] = mel_l; p.out[1] = l1; p.out[2] = l2; p.out[3] = l3;
        p.out[4] = 10.0f * mel_l + 2.0f * l1 + 2.0f * l2 + l3;
        p.partial[0] = n_el;              // hand the counts to the gradient kernel (stream order)
        p.partial[1] = n_ph;
    }
}
static __global__ void train_loss_grad_kernel(const LossP p) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nm = (long)p.B * p.L * p.n_mel, np_ = (long)p.B * p.T;
    const float n_el = p.partial[0], n_ph = p.partial[1];
    const float seed = p.grad_seed ? p.grad_seed[0] : 1.0f;
    if (q < nm) {
        const bool ok = !(p.mel_mask && p.mel_mask[q / p.n_mel]);
        const float d = p.mel_pred[q] - p.mel[q];
        p.d_mel[q] = ok ? (10.0f * (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f)) / n_el) * seed : 0.0f;
    }
    if (q < np_) {
        const bool ok = !(p.ph_mask && p.ph_mask[q]);
        const float d1 = p.pitch_pred[q] - p.pitch[q], d2 = p.energy_pred[q] - p.energy[q];
        const float d3 = logf(p.dur_pred[q] + 1.0f) - logf((float)p.dur[q] + 1.0f);
        p.d_pitch[q] = ok ? (2.0f * 2.0f * d1 / n_ph) * seed : 0.0f;
        p.d_energy[q] = ok ? (2.0f * 2.0f * d2 / n_ph) * seed : 0.0f;
        p.d_dur[q] = ok ? (2.0f * d3 / (p.dur_pred[q] + 1.0f) / n_ph) * seed : 0.0f;
    }
}

}  // namespace esmi
