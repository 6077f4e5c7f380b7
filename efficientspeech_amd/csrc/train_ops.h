// Training-step operators (model.py:167-226, 279-283): forward ops that keep what backward reads, their data-
// and weight-gradient kernels, the fused masked loss and AdamW -- one header per operator family, all of them kernels of the one
// translation unit tu_train.hip (no other unit includes these headers).
//
// Layouts: channels-last activations (B, n, C); weights in CHECKPOINT layout, what the optimizer updates (train_conv.h).
//
// Where the arithmetic runs.  On the matrix pipe: the dense weight gradient (train_wgrad.h train_conv_wgrad_mfma_kernel, a split-K
// MFMA reduction with a two-trip software pipeline); the dense forward and data gradients run there too, but through convgemm.h /
// pwgemm.h, not through these headers.  Everything else is fp32 FMA on the vector pipe: LDS-staged attention (train_attn.h),
// register-resident LayerNorm (train_norm.h), and one-thread-per-output kernels for the rest and as the fallback of every family.
//
// The contract: EVERY SUM RUNS IN A FIXED ORDER.
//   - Inside a wave and a workgroup: xor butterflies over fixed lane distances, trees over fixed strides, waves added in wave order
//     through LDS (train_reduce.h holds the vocabulary; nothing here adds in arrival order).
//   - Over the rows (B * n positions): two stages.  A first-stage kernel gives every (output element, chunk of rows) one partial sum,
//     added in row order; train_reduce_chunks_kernel / train_reduce_batch_kernel add an element's partials in chunk order.  The chunk
//     sizes depend on the shapes alone (tu_train.hip wgrad_plan), never on the device's state.
//   - ONE atomic: the atomicMax in train_conv_wgrad_mfma_kernel, max |dy| as the integer bit pattern of the magnitude.  An integer
//     max is order-independent, so it gives the same bits whatever order the workgroups arrive in.
// So the same inputs, shapes and library give the same bits on every run and every replay of a captured graph: a step is bitwise
// reproducible.  What that does NOT cover: another build (libesmi_fp32mfma.so forms its products differently), another shape or
// batch composition (other chunks, another association), another device generation, and torch's own kernels outside this library.
#pragma once
#include "train_reduce.h"   // the shared reductions, the second stage, column sums
#include "train_conv.h"     // ConvDesc; scalar forward / data gradient, depthwise, weight pack
#include "train_wgrad.h"    // weight gradients: scalar, depthwise, matrix pipe; the one-channel Linear's backward
#include "train_norm.h"     // LayerNorm forward / backward, activations
#include "train_attn.h"     // attention core forward / backward, global-memory and LDS-staged
#include "train_seq.h"      // embedding, masks, add, cat, length regulator
#include "train_loss.h"     // the masked loss and its gradient seeds
#include "train_optim.h"    // AdamW, step bookkeeping, gradient norm
