"""Which kernels one training step launches (CPU, wave simulator): the training-side twin of tests/test_dispatch.py.

The parity tests of the training step pass whichever kernels a shape lands on, so a slip in its host-side dispatch
(efficientspeech_amd/train.py, csrc/tu_train.hip) shows up only as a slowdown.  Each row below runs ONE step of a freshly built net
and pins (a) the kernels in launch order, written run-length (`6x name`), and (b) a digest of the complete launch records -- name,
grid, block, LDS bytes -- so that a change of chunking or of a workspace layout is caught as well as a change of kernel.

Below the rows, `test_schedule_across_the_option_matrix` pins what follows the micro-batch -- the accumulate launch and the window's
boundary -- for every combination of precision, clipping, accumulation and the weight average, by rule, with nothing recorded.

To re-record after an intended change of the launches: `python -m tests.test_train_dispatch` prints the table.
"""
import functools
import hashlib
import itertools
import os
import textwrap

import pytest

from tests.simlib import launch_records, sim_lib, use_sim
from tests.test_train_step import GOLD_SMALL, _setup, fused_conv_ln


def _fp32():
    train, _, net, x, y = _setup("cpu")
    return lambda: train.TrainStep(net).step(x, y)


def _precision16():
    """(the device-side optimizer that a captured step uses, esmi_train_adamw_graph_f32, runs here: hipGraph capture itself cannot
    run on the simulator)"""
    train, _, net, x, y = _setup("cpu")
    return lambda: train.TrainStep(net, precision=16).step(x, y)


def _fused_norm():
    train, _, net, x, y = _setup("cpu")

    def go():
        with fused_conv_ln(train):
            train.TrainStep(net).step(x, y)
    return go


def _plain_kernels():
    train, _, net, x, y = _setup("cpu")

    def go():
        train.USE_MATRIX_PIPE = False
        try:
            train.TrainStep(net).step(x, y)
        finally:
            train.USE_MATRIX_PIPE = True
    return go


def _small():
    train, _, net, x, y = _setup("cpu", GOLD_SMALL)
    return lambda: train.TrainStep(net).step(x, y)


def _synthetic():
    """B = 4, 48 phonemes, 192 frames: the dense weight gradients take train_conv_wgrad_mfma_kernel, the branch any realistic batch
    (and the benchmark) runs; the short fixture batch sends most of them to train_conv_wgrad_kernel + train_colsum_kernel."""
    train, _, net, _, _ = _setup("cpu")
    x, y = train.synthetic_batch(4, 48, 4, "cpu")
    return lambda: train.TrainStep(net).step(x, y)


def _outside_a_step():
    """training_loss + backward without the step's context (tests.test_train_step.check_loss_and_gradients): fresh gradient tensors,
    nothing deferred, nothing pre-packed."""
    train, _, net, x, y = _setup("cpu")
    train.TrainStep(net).flat.zero_grad()

    def go():
        _, total = train.training_loss(net, x, y)
        total.backward()
    return go


# row -> (set-up returning the call to log, number of launches, digest of the raw records, the kernels in launch order)
ROWS = {
    "fixture-fp32": (_fp32, 219, "e92201b491a1dfaa",
        "train_pack_batch_kernel train_embed_fwd_kernel convgemm_dma_kernel<4,1,NWV,false,false> convgemm_kernel<1,false> "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_attn_fwd_lds_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> 2x "
        "convgemm_kernel<1,false> train_act_fwd_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> 2x "
        "convgemm_kernel<1,false> pool_mask_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_attn_fwd_lds_kernel "
        "convgemm_kernel<1,false> train_ln_fwd4_kernel<16> 2x convgemm_kernel<1,false> train_act_fwd_kernel "
        "convgemm_kernel<1,false> train_ln_fwd4_kernel<16> 3x convgemm_kernel<1,false> train_cat_kernel "
        "convgemm_kernel<1,false> train_mask_rows_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> "
        "convgemm_kernel<1,false> conv_to1_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> convgemm_kernel<1,false> "
        "conv_to1_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> convgemm_kernel<1,false> conv_to1_kernel "
        "train_ln_fwd4_kernel<8> bucket_embed_kernel train_embed_fwd_kernel bucket_embed_kernel train_embed_fwd_kernel "
        "train_cat_kernel length_regulate_kernel train_repeat_fwd4_kernel pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> "
        "train_conv_dw_kernel pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_kernel<8,2,false> "
        "2x train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> "
        "train_conv_dw_kernel pwgemm_kernel<8,2,false> 2x train_ln_fwd4_kernel<32> pwgemm_kernel<8,2,false> "
        "train_loss_partial_kernel train_loss_final_kernel train_loss_grad_kernel train_conv_wgrad_mfma_kernel<false> "
        "pwgemm_kernel<5,2,false> 2x train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> "
        "train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> "
        "pwgemm_kernel<8,2,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel 2x train_ln_bwd4_kernel<32> "
        "train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel "
        "train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> "
        "train_repeat_bwd_kernel train_cat_kernel 2x train_embed_bwd_kernel train_ln_bwd4_kernel<8> train_act_bwd_kernel "
        "train_lin1_bwd4_kernel<8> train_act_bwd_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_lin1_bwd4_kernel<8> train_act_bwd_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel train_lin1_bwd4_kernel<8> train_act_bwd_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<8> absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_mask_rows_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_cat_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_ln_bwd4_kernel<16> absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_act_bwd_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel "
        "train_ln_bwd4_kernel<16> absmax_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel train_act_bwd_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_batch_kernel train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel absmax_kernel convgemm_dma_kernel<4,1,NWV,false,false> "
        "train_conv_wgrad_kernel absmax_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel "
        "train_embed_bwd_kernel train_reduce_batch_kernel train_adamw_kernel "),
    "fixture-precision16": (_precision16, 221, "84e665141149eeac",
        "train_pack_batch_kernel train_embed_fwd_kernel convgemm_dma_kernel<4,1,NWV,true,false> convgemm_kernel<1,true> "
        "convgemm_dma_kernel<4,1,NWV,true,false> train_attn_fwd_lds_kernel convgemm_kernel<1,true> train_ln_fwd4_kernel<8> 2x "
        "convgemm_kernel<1,true> train_act_fwd_kernel convgemm_kernel<1,true> train_ln_fwd4_kernel<8> 2x "
        "convgemm_kernel<1,true> pool_mask_kernel convgemm_dma_kernel<4,1,NWV,true,false> train_attn_fwd_lds_kernel "
        "convgemm_kernel<1,true> train_ln_fwd4_kernel<16> 2x convgemm_kernel<1,true> train_act_fwd_kernel "
        "convgemm_kernel<1,true> train_ln_fwd4_kernel<16> 3x convgemm_kernel<1,true> train_cat_kernel convgemm_kernel<1,true> "
        "train_mask_rows_kernel convgemm_kernel<1,true> train_ln_fwd4_kernel<8> convgemm_kernel<1,true> conv_to1_kernel "
        "convgemm_kernel<1,true> train_ln_fwd4_kernel<8> convgemm_kernel<1,true> conv_to1_kernel convgemm_kernel<1,true> "
        "train_ln_fwd4_kernel<8> convgemm_kernel<1,true> conv_to1_kernel train_ln_fwd4_kernel<8> bucket_embed_kernel "
        "train_embed_fwd_kernel bucket_embed_kernel train_embed_fwd_kernel train_cat_kernel length_regulate_kernel "
        "train_repeat_fwd4_kernel pwgemm_kernel<8,2,true> train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_kernel<8,2,true> "
        "train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_kernel<8,2,true> 2x train_ln_fwd4_kernel<32> train_conv_dw_kernel "
        "pwgemm_kernel<8,2,true> train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_kernel<8,2,true> 2x "
        "train_ln_fwd4_kernel<32> pwgemm_kernel<8,2,true> train_loss_partial_kernel train_loss_final_kernel "
        "train_loss_grad_kernel train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<5,2,true> 2x train_ln_bwd4_kernel<32> "
        "train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,true> train_conv_dw_kernel train_conv_wgrad_dw4_kernel "
        "train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,true> train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel 2x train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,true> "
        "train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> "
        "pwgemm_kernel<8,2,true> train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> "
        "train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,true> train_repeat_bwd_kernel train_cat_kernel 2x "
        "train_embed_bwd_kernel train_ln_bwd4_kernel<8> train_act_bwd_kernel train_lin1_bwd4_kernel<8> train_act_bwd_kernel "
        "absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<8> "
        "absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel train_lin1_bwd4_kernel<8> "
        "train_act_bwd_kernel absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel "
        "train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel "
        "train_lin1_bwd4_kernel<8> train_act_bwd_kernel absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel "
        "train_colsum_kernel train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel "
        "train_colsum_kernel train_mask_rows_kernel absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel "
        "train_colsum_kernel train_cat_kernel absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel "
        "absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel absmax_kernel "
        "convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<16> absmax_kernel "
        "convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel train_act_bwd_kernel absmax_kernel "
        "convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel absmax_kernel convgemm_kernel<1,true> "
        "train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<16> absmax_kernel "
        "convgemm_dma_kernel<4,1,NWV,true,false> train_conv_wgrad_kernel train_colsum_kernel train_attn_bwd_rows_lds_kernel "
        "train_attn_bwd_cols_kernel absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel absmax_kernel "
        "convgemm_kernel<1,true> train_conv_wgrad_kernel absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel "
        "train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel "
        "train_act_bwd_kernel absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel absmax_kernel "
        "convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel train_reduce_batch_kernel train_ln_bwd4_kernel<8> "
        "absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel train_colsum_kernel train_attn_bwd_rows_lds_kernel "
        "train_attn_bwd_cols_kernel absmax_kernel convgemm_kernel<1,true> train_conv_wgrad_kernel absmax_kernel "
        "convgemm_dma_kernel<4,1,NWV,true,false> train_conv_wgrad_kernel absmax_kernel convgemm_dma_kernel<4,1,NWV,true,false> "
        "train_conv_wgrad_kernel train_embed_bwd_kernel train_reduce_batch_kernel absmax_kernel train_bump_step_kernel "
        "train_adamw_dev_kernel "),
    "fixture-fused-norm": (_fused_norm, 207, "282447a48f9d699b",
        "train_pack_batch_kernel train_embed_fwd_kernel convgemm_dma_kernel<4,1,NWV,false,false> convgemm_kernel<1,false> "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_attn_fwd_lds_kernel 3x convgemm_kernel<1,false> train_act_fwd_kernel 3x "
        "convgemm_kernel<1,false> pool_mask_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_attn_fwd_lds_kernel "
        "convgemm_kernel<2,false> 2x convgemm_kernel<1,false> train_act_fwd_kernel convgemm_kernel<2,false> 3x "
        "convgemm_kernel<1,false> train_cat_kernel convgemm_kernel<1,false> train_mask_rows_kernel 2x convgemm_kernel<1,false> "
        "conv_to1_kernel 2x convgemm_kernel<1,false> conv_to1_kernel 2x convgemm_kernel<1,false> conv_to1_kernel "
        "train_ln_fwd4_kernel<8> bucket_embed_kernel train_embed_fwd_kernel bucket_embed_kernel train_embed_fwd_kernel "
        "train_cat_kernel length_regulate_kernel train_repeat_fwd4_kernel pwgemm_kernel<8,4,false> train_conv_dw_kernel "
        "pwgemm_kernel<8,4,false> train_conv_dw_kernel pwgemm_kernel<8,4,false> train_ln_fwd4_kernel<32> train_conv_dw_kernel "
        "pwgemm_kernel<8,4,false> train_conv_dw_kernel pwgemm_kernel<8,4,false> train_ln_fwd4_kernel<32> "
        "pwgemm_kernel<8,2,false> train_loss_partial_kernel train_loss_final_kernel train_loss_grad_kernel "
        "train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<5,2,false> 2x train_ln_bwd4_kernel<32> "
        "train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel "
        "train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel 2x train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> "
        "train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> "
        "pwgemm_kernel<8,2,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> "
        "train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> train_repeat_bwd_kernel train_cat_kernel 2x "
        "train_embed_bwd_kernel train_ln_bwd4_kernel<8> train_act_bwd_kernel train_lin1_bwd4_kernel<8> train_act_bwd_kernel "
        "absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<8> "
        "absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_lin1_bwd4_kernel<8> "
        "train_act_bwd_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel "
        "train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel "
        "train_lin1_bwd4_kernel<8> train_act_bwd_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_mask_rows_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_cat_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<16> absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_act_bwd_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<16> absmax_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel train_colsum_kernel train_attn_bwd_rows_lds_kernel "
        "train_attn_bwd_cols_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_ln_bwd4_kernel<8> absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel "
        "train_act_bwd_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_reduce_batch_kernel train_ln_bwd4_kernel<8> "
        "absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_attn_bwd_rows_lds_kernel "
        "train_attn_bwd_cols_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel absmax_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel absmax_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel train_embed_bwd_kernel train_reduce_batch_kernel "
        "train_adamw_kernel "),
    "fixture-plain-kernels": (_plain_kernels, 248, "77ce8619201129f5",
        "train_embed_fwd_kernel 3x train_conv_fwd_kernel train_attn_fwd_lds_kernel train_conv_fwd_kernel "
        "train_ln_fwd4_kernel<8> 2x train_conv_fwd_kernel train_act_fwd_kernel train_conv_fwd_kernel train_ln_fwd4_kernel<8> 2x "
        "train_conv_fwd_kernel pool_mask_kernel train_conv_fwd_kernel train_attn_fwd_lds_kernel train_conv_fwd_kernel "
        "train_ln_fwd4_kernel<16> 2x train_conv_fwd_kernel train_act_fwd_kernel train_conv_fwd_kernel train_ln_fwd4_kernel<16> "
        "3x train_conv_fwd_kernel train_cat_kernel train_conv_fwd_kernel train_mask_rows_kernel train_conv_fwd_kernel "
        "train_act_fwd_kernel train_ln_fwd4_kernel<8> train_conv_fwd_kernel train_act_fwd_kernel 2x train_conv_fwd_kernel "
        "train_act_fwd_kernel train_ln_fwd4_kernel<8> train_conv_fwd_kernel train_act_fwd_kernel 2x train_conv_fwd_kernel "
        "train_act_fwd_kernel train_ln_fwd4_kernel<8> train_conv_fwd_kernel train_act_fwd_kernel train_conv_fwd_kernel "
        "train_act_fwd_kernel train_ln_fwd4_kernel<8> bucket_embed_kernel train_embed_fwd_kernel bucket_embed_kernel "
        "train_embed_fwd_kernel train_cat_kernel length_regulate_kernel train_repeat_fwd4_kernel train_conv_fwd_kernel "
        "train_act_fwd_kernel train_ln_fwd4_kernel<32> train_conv_dw_kernel train_conv_fwd_kernel train_act_fwd_kernel "
        "train_ln_fwd4_kernel<32> train_conv_dw_kernel train_conv_fwd_kernel train_act_fwd_kernel 2x train_ln_fwd4_kernel<32> "
        "train_conv_dw_kernel train_conv_fwd_kernel train_act_fwd_kernel train_ln_fwd4_kernel<32> train_conv_dw_kernel "
        "train_conv_fwd_kernel train_act_fwd_kernel 2x train_ln_fwd4_kernel<32> train_conv_fwd_kernel train_loss_partial_kernel "
        "train_loss_final_kernel train_loss_grad_kernel train_conv_dgrad_kernel train_conv_wgrad_mfma_kernel<false> "
        "train_reduce_chunks_kernel 2x train_ln_bwd4_kernel<32> train_conv_dgrad_kernel train_conv_wgrad_mfma_kernel<false> "
        "train_reduce_chunks_kernel train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_reduce_chunks_kernel "
        "train_ln_bwd4_kernel<32> train_conv_dgrad_kernel train_conv_wgrad_mfma_kernel<false> train_reduce_chunks_kernel "
        "train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_reduce_chunks_kernel 2x train_ln_bwd4_kernel<32> "
        "train_conv_dgrad_kernel train_conv_wgrad_mfma_kernel<false> train_reduce_chunks_kernel train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel train_reduce_chunks_kernel train_ln_bwd4_kernel<32> train_conv_dgrad_kernel "
        "train_conv_wgrad_mfma_kernel<false> train_reduce_chunks_kernel train_conv_dw_kernel train_conv_wgrad_dw4_kernel "
        "train_reduce_chunks_kernel train_ln_bwd4_kernel<32> train_conv_dgrad_kernel train_conv_wgrad_mfma_kernel<false> "
        "train_reduce_chunks_kernel train_repeat_bwd_kernel train_cat_kernel 2x train_embed_bwd_kernel train_ln_bwd4_kernel<8> "
        "train_act_bwd_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel "
        "train_act_bwd_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel "
        "train_ln_bwd4_kernel<8> train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel "
        "train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_act_bwd_kernel "
        "train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_ln_bwd4_kernel<8> "
        "train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_conv_dgrad_kernel "
        "train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_act_bwd_kernel train_conv_dgrad_kernel "
        "train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_ln_bwd4_kernel<8> train_conv_dgrad_kernel "
        "train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_mask_rows_kernel train_conv_dgrad_kernel "
        "train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_cat_kernel train_conv_dgrad_kernel "
        "train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_chunks_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel "
        "train_reduce_chunks_kernel train_ln_bwd4_kernel<16> train_conv_dgrad_kernel train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_chunks_kernel train_act_bwd_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_chunks_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel "
        "train_reduce_chunks_kernel train_ln_bwd4_kernel<16> train_conv_dgrad_kernel train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_chunks_kernel train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel "
        "train_conv_dgrad_kernel train_conv_wgrad_kernel train_reduce_chunks_kernel train_conv_dgrad_kernel "
        "train_conv_wgrad_kernel train_reduce_chunks_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel "
        "train_reduce_chunks_kernel train_ln_bwd4_kernel<8> train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel "
        "train_reduce_chunks_kernel train_act_bwd_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel "
        "train_reduce_chunks_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel "
        "train_reduce_chunks_kernel train_ln_bwd4_kernel<8> train_conv_dgrad_kernel train_conv_wgrad_kernel train_colsum_kernel "
        "train_reduce_chunks_kernel train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel train_conv_dgrad_kernel "
        "train_conv_wgrad_kernel train_reduce_chunks_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel "
        "train_reduce_chunks_kernel train_conv_dgrad_kernel train_conv_wgrad_kernel train_reduce_chunks_kernel "
        "train_embed_bwd_kernel train_reduce_batch_kernel train_adamw_kernel "),
    "small-fixture": (_small, 237, "2184d7050be6cd48",
        "train_pack_batch_kernel train_embed_fwd_kernel convgemm_dma_kernel<4,1,NWV,false,false> convgemm_kernel<1,false> "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_attn_fwd_lds_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<16> "
        "2x convgemm_kernel<1,false> train_act_fwd_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<16> "
        "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,false> pool_mask_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_attn_fwd_lds_kernel convgemm_dma_kernel<4,1,NWV,false,false> "
        "train_ln_fwd4_kernel<32> pwgemm_kernel<8,2,false> convgemm_dma_kernel<4,1,NWV,false,false> train_act_fwd_kernel "
        "pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> 3x convgemm_kernel<1,false> train_cat_kernel "
        "convgemm_kernel<1,false> train_mask_rows_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<16> "
        "convgemm_kernel<1,false> conv_to1_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<16> convgemm_kernel<1,false> "
        "conv_to1_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<16> convgemm_kernel<1,false> conv_to1_kernel "
        "train_ln_fwd4_kernel<16> bucket_embed_kernel train_embed_fwd_kernel bucket_embed_kernel train_embed_fwd_kernel "
        "train_cat_kernel length_regulate_kernel train_repeat_fwd4_kernel convgemm_dma_kernel<4,1,NWV,false,false> "
        "train_ln_fwd4_kernel<64> train_conv_dw_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_ln_fwd4_kernel<64> "
        "train_conv_dw_kernel convgemm_dma_kernel<4,1,NWV,false,false> 2x train_ln_fwd4_kernel<64> train_conv_dw_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_ln_fwd4_kernel<64> train_conv_dw_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> 2x train_ln_fwd4_kernel<64> train_conv_dw_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_ln_fwd4_kernel<64> train_conv_dw_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> 2x train_ln_fwd4_kernel<64> convgemm_dma_kernel<4,1,NWV,false,false> "
        "train_loss_partial_kernel train_loss_final_kernel train_loss_grad_kernel train_conv_wgrad_mfma_kernel<false> "
        "convgemm_kernel<1,false> 2x train_ln_bwd_fused_kernel train_conv_wgrad_mfma_kernel<false> "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd_fused_kernel "
        "train_conv_wgrad_mfma_kernel<false> convgemm_dma_kernel<4,1,NWV,false,false> train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel 2x train_ln_bwd_fused_kernel train_conv_wgrad_mfma_kernel<false> "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd_fused_kernel "
        "train_conv_wgrad_mfma_kernel<false> convgemm_dma_kernel<4,1,NWV,false,false> train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel 2x train_ln_bwd_fused_kernel train_conv_wgrad_mfma_kernel<false> "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd_fused_kernel "
        "train_conv_wgrad_mfma_kernel<false> convgemm_dma_kernel<4,1,NWV,false,false> train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel train_ln_bwd_fused_kernel train_conv_wgrad_mfma_kernel<false> "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_repeat_bwd_kernel train_cat_kernel 2x train_embed_bwd_kernel "
        "train_ln_bwd4_kernel<16> train_act_bwd_kernel train_lin1_bwd4_kernel<16> train_act_bwd_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<16> absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_lin1_bwd4_kernel<16> train_act_bwd_kernel "
        "absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<16> "
        "absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_lin1_bwd4_kernel<16> "
        "train_act_bwd_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel "
        "train_ln_bwd4_kernel<16> absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel "
        "train_mask_rows_kernel absmax_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_cat_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel absmax_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel train_colsum_kernel "
        "absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<32> "
        "absmax_kernel pwgemm_kernel<8,2,false> train_conv_wgrad_kernel train_colsum_kernel train_act_bwd_kernel absmax_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel train_colsum_kernel absmax_kernel "
        "pwgemm_kernel<8,2,false> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<32> absmax_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel train_colsum_kernel train_reduce_batch_kernel "
        "train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel absmax_kernel convgemm_dma_kernel<4,1,NWV,false,false> "
        "train_conv_wgrad_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_ln_bwd4_kernel<16> absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel train_act_bwd_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_ln_bwd4_kernel<16> absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel absmax_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel absmax_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel train_embed_bwd_kernel train_reduce_batch_kernel "
        "train_adamw_kernel "),
    "synthetic-B4-T48": (_synthetic, 177, "987736f70deb4de4",
        "train_pack_batch_kernel train_embed_fwd_kernel convgemm_dma_kernel<4,1,NWV,false,false> convgemm_kernel<1,false> "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_attn_fwd_lds_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> 2x "
        "convgemm_kernel<1,false> train_act_fwd_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> 2x "
        "convgemm_kernel<1,false> pool_mask_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_attn_fwd_lds_kernel "
        "convgemm_kernel<1,false> train_ln_fwd4_kernel<16> 2x convgemm_kernel<1,false> train_act_fwd_kernel "
        "convgemm_kernel<1,false> train_ln_fwd4_kernel<16> 3x convgemm_kernel<1,false> train_cat_kernel "
        "convgemm_kernel<1,false> train_mask_rows_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> "
        "convgemm_kernel<1,false> conv_to1_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> convgemm_kernel<1,false> "
        "conv_to1_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> convgemm_kernel<1,false> conv_to1_kernel "
        "train_ln_fwd4_kernel<8> bucket_embed_kernel train_embed_fwd_kernel bucket_embed_kernel train_embed_fwd_kernel "
        "train_cat_kernel length_regulate_kernel train_repeat_fwd4_kernel pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> "
        "train_conv_dw_kernel pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_kernel<8,2,false> "
        "2x train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> "
        "train_conv_dw_kernel pwgemm_kernel<8,2,false> 2x train_ln_fwd4_kernel<32> pwgemm_kernel<8,2,false> "
        "train_loss_partial_kernel train_loss_final_kernel train_loss_grad_kernel train_conv_wgrad_mfma_kernel<false> "
        "pwgemm_kernel<5,2,false> 2x train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> "
        "train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> "
        "pwgemm_kernel<8,2,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel 2x train_ln_bwd4_kernel<32> "
        "train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel "
        "train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_kernel<8,2,false> "
        "train_repeat_bwd_kernel train_cat_kernel 2x train_embed_bwd_kernel train_ln_bwd4_kernel<8> train_act_bwd_kernel "
        "train_lin1_bwd4_kernel<8> train_act_bwd_kernel train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> "
        "train_ln_bwd4_kernel<8> train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_lin1_bwd4_kernel<8> "
        "train_act_bwd_kernel train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_ln_bwd4_kernel<8> "
        "train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_lin1_bwd4_kernel<8> train_act_bwd_kernel "
        "train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_ln_bwd4_kernel<8> "
        "train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_mask_rows_kernel "
        "train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_cat_kernel train_conv_wgrad_mfma_kernel<true> "
        "convgemm_kernel<1,false> train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> "
        "train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_ln_bwd4_kernel<16> "
        "train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_act_bwd_kernel train_conv_wgrad_mfma_kernel<false> "
        "convgemm_kernel<1,false> train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_ln_bwd4_kernel<16> "
        "train_conv_wgrad_mfma_kernel<false> convgemm_dma_kernel<4,1,NWV,false,false> train_attn_bwd_rows_lds_kernel "
        "train_attn_bwd_cols_kernel train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> "
        "train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_conv_wgrad_mfma_kernel<false> "
        "convgemm_kernel<1,false> train_ln_bwd4_kernel<8> train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> "
        "train_act_bwd_kernel train_conv_wgrad_mfma_kernel<false> convgemm_kernel<1,false> train_conv_wgrad_mfma_kernel<false> "
        "train_reduce_batch_kernel convgemm_kernel<1,false> train_ln_bwd4_kernel<8> train_conv_wgrad_mfma_kernel<false> "
        "convgemm_kernel<1,false> train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel train_conv_wgrad_mfma_kernel<false> "
        "convgemm_kernel<1,false> train_conv_wgrad_mfma_kernel<false> convgemm_dma_kernel<4,1,NWV,false,false> "
        "train_conv_wgrad_mfma_kernel<false> convgemm_dma_kernel<4,1,NWV,false,false> train_embed_bwd_kernel "
        "train_reduce_batch_kernel train_adamw_kernel "),
    "outside-a-step": (_outside_a_step, 310, "528396313f013f7d",
        "train_embed_fwd_kernel pack_conv_kernel convgemm_dma_kernel<4,1,NWV,false,false> convgemm_kernel<1,false> "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_attn_fwd_lds_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> "
        "convgemm_kernel<1,false> pack_conv_kernel convgemm_kernel<1,false> train_act_fwd_kernel convgemm_kernel<1,false> "
        "train_ln_fwd4_kernel<8> 2x convgemm_kernel<1,false> pool_mask_kernel convgemm_dma_kernel<4,1,NWV,false,false> "
        "train_attn_fwd_lds_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<16> convgemm_kernel<1,false> pack_conv_kernel "
        "convgemm_kernel<1,false> train_act_fwd_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<16> 2x "
        "convgemm_kernel<1,false> pack_conv_kernel convgemm_kernel<1,false> train_cat_kernel convgemm_kernel<1,false> "
        "train_mask_rows_kernel pack_conv_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> pack_conv_kernel "
        "convgemm_kernel<1,false> conv_to1_kernel pack_conv_kernel convgemm_kernel<1,false> train_ln_fwd4_kernel<8> "
        "pack_conv_kernel convgemm_kernel<1,false> conv_to1_kernel pack_conv_kernel convgemm_kernel<1,false> "
        "train_ln_fwd4_kernel<8> pack_conv_kernel convgemm_kernel<1,false> conv_to1_kernel train_ln_fwd4_kernel<8> "
        "bucket_embed_kernel train_embed_fwd_kernel bucket_embed_kernel train_embed_fwd_kernel train_cat_kernel "
        "length_regulate_kernel train_repeat_fwd4_kernel pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> train_conv_dw_kernel "
        "pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_kernel<8,2,false> 2x "
        "train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_kernel<8,2,false> train_ln_fwd4_kernel<32> train_conv_dw_kernel "
        "pwgemm_kernel<8,2,false> 2x train_ln_fwd4_kernel<32> pwgemm_kernel<8,2,false> train_loss_partial_kernel "
        "train_loss_final_kernel train_loss_grad_kernel pack_conv_kernel train_conv_wgrad_mfma_kernel<false> "
        "train_reduce_chunks_kernel pwgemm_kernel<5,2,false> train_ln_bwd4_kernel<32> train_reduce_chunks_kernel "
        "train_ln_bwd4_kernel<32> train_reduce_chunks_kernel pack_conv_kernel train_conv_wgrad_mfma_kernel<false> "
        "train_reduce_chunks_kernel pwgemm_kernel<8,2,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel "
        "train_reduce_chunks_kernel train_ln_bwd4_kernel<32> train_reduce_chunks_kernel pack_conv_kernel "
        "train_conv_wgrad_mfma_kernel<false> train_reduce_chunks_kernel pwgemm_kernel<8,2,false> train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel train_reduce_chunks_kernel train_ln_bwd4_kernel<32> train_reduce_chunks_kernel "
        "train_ln_bwd4_kernel<32> train_reduce_chunks_kernel pack_conv_kernel train_conv_wgrad_mfma_kernel<false> "
        "train_reduce_chunks_kernel pwgemm_kernel<8,2,false> train_conv_dw_kernel train_conv_wgrad_dw4_kernel "
        "train_reduce_chunks_kernel train_ln_bwd4_kernel<32> train_reduce_chunks_kernel pack_conv_kernel "
        "train_conv_wgrad_mfma_kernel<false> train_reduce_chunks_kernel pwgemm_kernel<8,2,false> train_conv_dw_kernel "
        "train_conv_wgrad_dw4_kernel train_reduce_chunks_kernel train_ln_bwd4_kernel<32> train_reduce_chunks_kernel "
        "pack_conv_kernel train_conv_wgrad_mfma_kernel<false> train_reduce_chunks_kernel pwgemm_kernel<8,2,false> "
        "train_repeat_bwd_kernel train_cat_kernel train_embed_bwd_kernel train_reduce_chunks_kernel train_embed_bwd_kernel "
        "train_reduce_chunks_kernel train_ln_bwd4_kernel<8> train_reduce_chunks_kernel train_act_bwd_kernel "
        "train_lin1_bwd4_kernel<8> train_reduce_chunks_kernel train_act_bwd_kernel pack_conv_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel "
        "train_ln_bwd4_kernel<8> train_reduce_chunks_kernel pack_conv_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_lin1_bwd4_kernel<8> "
        "train_reduce_chunks_kernel train_act_bwd_kernel pack_conv_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_ln_bwd4_kernel<8> "
        "train_reduce_chunks_kernel pack_conv_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_chunks_kernel train_lin1_bwd4_kernel<8> train_reduce_chunks_kernel "
        "train_act_bwd_kernel pack_conv_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_chunks_kernel train_ln_bwd4_kernel<8> train_reduce_chunks_kernel pack_conv_kernel "
        "absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel "
        "train_mask_rows_kernel pack_conv_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_chunks_kernel train_cat_kernel pack_conv_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel pack_conv_kernel "
        "absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel "
        "pack_conv_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel "
        "train_reduce_chunks_kernel train_ln_bwd4_kernel<16> train_reduce_chunks_kernel pack_conv_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_act_bwd_kernel "
        "pack_conv_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel "
        "train_reduce_chunks_kernel pack_conv_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_chunks_kernel train_ln_bwd4_kernel<16> train_reduce_chunks_kernel pack_conv_kernel "
        "absmax_kernel convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel train_colsum_kernel "
        "train_reduce_chunks_kernel train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel pack_conv_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_reduce_chunks_kernel pack_conv_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_reduce_chunks_kernel pack_conv_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_reduce_chunks_kernel train_ln_bwd4_kernel<8> "
        "train_reduce_chunks_kernel pack_conv_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_colsum_kernel train_reduce_chunks_kernel train_act_bwd_kernel pack_conv_kernel absmax_kernel "
        "convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel pack_conv_kernel "
        "absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel "
        "train_ln_bwd4_kernel<8> train_reduce_chunks_kernel pack_conv_kernel absmax_kernel convgemm_kernel<1,false> "
        "train_conv_wgrad_kernel train_colsum_kernel train_reduce_chunks_kernel train_attn_bwd_rows_lds_kernel "
        "train_attn_bwd_cols_kernel pack_conv_kernel absmax_kernel convgemm_kernel<1,false> train_conv_wgrad_kernel "
        "train_reduce_chunks_kernel pack_conv_kernel absmax_kernel convgemm_dma_kernel<4,1,NWV,false,false> "
        "train_conv_wgrad_kernel train_reduce_chunks_kernel pack_conv_kernel absmax_kernel "
        "convgemm_dma_kernel<4,1,NWV,false,false> train_conv_wgrad_kernel train_reduce_chunks_kernel train_embed_bwd_kernel "
        "train_reduce_chunks_kernel "),
}


def launch_log(setup):
    """the simulator's launch records (`name gx gy gz bx by bz lds`, one per line) of the call that `setup()` returns"""
    with use_sim():
        call = setup()
        lib = sim_lib()
        lib.wavesim_launch_log_clear()
        try:
            call()
            return lib.wavesim_launch_log().decode().splitlines()
        finally:
            lib.wavesim_launch_log_clear()


def summarize(records):
    """-> (number of launches, digest of the records, the names run-length encoded)"""
    names = []
    for rec in records:
        name = rec.rsplit(" ", 7)[0].replace(" ", "")      # (as tests.simlib.launched_kernels spells them)
        names.append(name[1:-1] if name.startswith("(") else name)
    runs = []
    for n in names:
        if runs and runs[-1][0] == n:
            runs[-1][1] += 1
        else:
            runs.append([n, 1])
    text = " ".join(n if k == 1 else f"{k}x {n}" for n, k in runs)
    return len(records), hashlib.sha256("\n".join(records).encode()).hexdigest()[:16], text


@pytest.mark.parametrize("row", list(ROWS))
def test_train_step_launches(row):
    setup, count, digest, expected = ROWS[row]
    got_count, got_digest, got = summarize(launch_log(setup))
    assert got.split() == expected.split()                 # which kernels, in which order
    assert (got_count, got_digest) == (count, digest)      # ... and every grid, block and LDS size


# ---------------------------------------------------------------------------------------------- the schedule across the option matrix
MATRIX = list(itertools.product((32, 16, "bf16"), (None, 1.0), (1, 2), (None, 0.9)))     # precision, clip, N, decay: the first of a precision is its base
LAST_OF_THE_MICRO_BATCH = "train_reduce_batch_kernel"


def _matrix_calls(precision, clip, n, decay):
    """-> the launch records of each of the N calls of `step` that fill one window; asserts the counters after every call."""
    train, _, net, x, y = _setup("cpu")
    kw = {"init_scale": 1024.0} if precision == 16 else {}
    step = train.TrainStep(net, precision=precision, gradient_clip_val=clip, accumulate_grad_batches=n, ema_decay=decay, **kw)
    calls = []
    for k in range(1, n + 1):
        with launch_records() as got:
            step.step(x, y)
        assert step.micro == k % n and step.t == (1 if k == n else 0), (k, step.micro, step.t)
        calls.append(got)
    return calls


def _split(records):
    names = [name for name, _ in records]
    at = len(names) - 1 - names[::-1].index(LAST_OF_THE_MICRO_BATCH)
    return records[:at], names[at:]


@functools.lru_cache(maxsize=None)
def _matrix_head(precision):
    """the records of a precision's first case (no clipping, N = 1, no average) in front of its last train_reduce_batch_kernel"""
    (records,) = _matrix_calls(precision, None, 1, None)
    return _split(records)[0]


def _boundary_names(precision, clip, decay):
    names = ["absmax_kernel"] if precision == 16 else []
    names += ["train_grad_sumsq_kernel"] if clip else []
    if precision == 16 or clip:                            # the optimizer's scalars on the device
        names += ["train_bump_clip_kernel" if clip else "train_bump_step_kernel", "train_adamw_dev_kernel"]
    else:
        names += ["train_adamw_kernel"]
    return names + (["train_ema_update_kernel"] if decay else [])


@pytest.mark.parametrize("precision,clip,n,decay", MATRIX, ids=lambda v: str(v))
def test_schedule_across_the_option_matrix(precision, clip, n, decay):
    """Every combination of precision, clipping, accumulation and the average: each of a window's N calls launches the base case's
    micro-batch record for record, then the accumulate launch when N > 1, and the N-th alone the boundary -- the scaler's reduction,
    the clipping's, the optimizer in its mode, the average's update, in this order and nothing else."""
    with use_sim():
        head = _matrix_head(precision)
        calls = _matrix_calls(precision, clip, n, decay)
    for k, records in enumerate(calls, 1):
        got_head, got_tail = _split(records)
        assert got_head == head, (k, len(got_head), len(head))
        want = [LAST_OF_THE_MICRO_BATCH] + (["train_grad_accumulate_kernel"] if n > 1 else [])
        assert got_tail == want + (_boundary_names(precision, clip, decay) if k == n else []), (k, got_tail)


if __name__ == "__main__":
    os.environ.setdefault("WAVESIM_THREADS", "16")
    for row, (setup, *_) in ROWS.items():
        count, digest, text = summarize(launch_log(setup))
        lines = textwrap.wrap(text, 118, break_long_words=False, break_on_hyphens=False)
        print(f'    "{row}": ({setup.__name__}, {count}, "{digest}",')
        print("\n".join(f'        "{ln} "' for ln in lines) + "),")
