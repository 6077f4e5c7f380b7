"""Which kernels the host-side dispatch launches, shape class by shape class (CPU, wave simulator).

Every encoder-side path is parity-equivalent by design, so the parity tests pass whichever kernels a shape lands on; a dispatch
mistake shows up only as a slowdown.  This table pins the launch sequence of the encoder-side selectors (esmi_encoder_block_f32,
the Fuse + variance-adaptor stage, the one-call forward's encoder side) for each shape class and launch plan.  Weight preparation
(packing, composing, range scans) is left out of the lists: it runs once per weight set, not per call.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from efficientspeech_amd import CONFIGS, _lib, build_phoneme2mel, load_numpy_state_dict
from efficientspeech_amd.synth import synth_phonemes, synth_state_dict
from oracle import oracle
from tests import helpers as H
from tests.simlib import launch_records, use_sim

_CONFIGS = {"tiny": CONFIGS["tiny"], "small": CONFIGS["small"], "base": CONFIGS["base"],
            "tiny_e2": dataclasses.replace(CONFIGS["tiny"], name="tiny_e2", expansion=2),      # MixFFN expansion 2 on dim 32
            "base_k3": dataclasses.replace(CONFIGS["base"], name="base_k3", kernel_size=3)}    # the reference's default kernel size
_NETS = {}
_PREP = ("pack_", "compose_merge_kernel", "absmax_kernel", "copy_pad_kernel")
_DEC = " mel_decoder_kernel<DX2,KD,NW>"

# (config, B, T, lengths, launch plan, entry point) -> the kernels launched, in order.  Entry points: "forward" = net(x), the one-call
# forward (esmi_phoneme2mel_forward_f32, decoder included); "encode" = net.encoder._encode(x), the module path (esmi_encoder_block_f32
# per block + esmi_fuse_variance_adaptor_f32); "block" = the encoder blocks alone through esmi_encoder_block_f32 with the MixFFN Linear
# not folded into the conv (ESMI_FOLD_FFN=0); "encode_no_ln2" = "encode" with the pitch and energy predictors' ln2_g / ln2_b NULL (esmi.h
# allows it: their LayerNorm 2 is never applied), which enc_pred128 would read -- that call takes the per-op predictors.
L40, L150 = [40, 23], [150, 97]
ROWS = [
    ("tiny", 2, 40, L40, 63, "forward",
     "enc_all16_kernel<4> max_i32_kernel" + _DEC),
    ("tiny", 2, 40, L40, 63, "encode",
     "enc_b0_16_kernel<4> enc_b1_16_kernel enc_va16_kernel<3> max_i32_kernel"),
    ("tiny", 2, 40, L40, 31, "forward",
     "enc_attn_ffn_kernel<2,1,1,4,3,1> enc_attn_ffn_split_kernel<2,2,1,1,1,2> enc_fuse_va_kernel<1,3> max_i32_kernel" + _DEC),
    ("tiny", 2, 40, L40, 31, "encode",
     "enc_attn_ffn_kernel<2,1,1,4,3,1> enc_attn_ffn_split_kernel<2,2,1,1,1,2> enc_fuse_va_kernel<1,3> max_i32_kernel"),
    ("tiny", 2, 40, L40, 23, "forward",
     "enc_attn_ffn_kernel<2,1,1,4,3,1> enc_attn_ffn_kernel<2,2,1,1,1,2> enc_fuse_va_kernel<1,3> max_i32_kernel" + _DEC),
    ("tiny", 2, 40, L40, 23, "encode",
     "enc_attn_ffn_kernel<2,1,1,4,3,1> enc_attn_ffn_kernel<2,2,1,1,1,2> enc_fuse_va_kernel<1,3> max_i32_kernel"),
    ("tiny", 2, 40, L40, 7, "forward",
     "enc_merge_qkv_kernel<4,1,3,1> enc_attn_ffn_kernel<2,1,1> enc_merge_qkv_kernel<1,2,1,2> enc_attn_ffn_kernel<2,2,1> "
     "enc_fuse_va_kernel<1,3> max_i32_kernel" + _DEC),
    ("tiny", 2, 40, L40, 7, "encode",
     "enc_merge_qkv_kernel<4,1,3,1> enc_attn_ffn_kernel<2,1,1> enc_merge_qkv_kernel<1,2,1,2> enc_attn_ffn_kernel<2,2,1> "
     "enc_fuse_va_kernel<1,3> max_i32_kernel"),
    ("tiny", 2, 40, L40, 0, "forward",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> attn_kernel<2> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> "
     "pool_mask_kernel attn_kernel<1> convgemm_kernel<2,false> convgemm_kernel<1,false> convgemm_kernel<2,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> va_tail_kernel length_regulate_kernel "
     "convgemm_dma_kernel<4,1,NWV,false,true> max_i32_kernel" + _DEC),
    ("tiny", 2, 40, L40, 0, "encode",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> attn_kernel<2> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> "
     "pool_mask_kernel attn_kernel<1> convgemm_kernel<2,false> convgemm_kernel<1,false> convgemm_kernel<2,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> va_tail_kernel length_regulate_kernel max_i32_kernel"),
    ("tiny", 2, 128, [128, 77], 63, "forward",
     "enc_all16_kernel<8> max_i32_kernel" + _DEC),
    ("tiny", 1, 31, None, 63, "forward",
     "enc_all16_kernel<2> max_i32_kernel" + _DEC),
    ("tiny", 2, 150, L150, 63, "forward",
     "enc_merge_qkv_kernel<4,1,3,1> attn_lds_kernel<8,32> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> enc_merge_qkv_kernel<1,2,1,2> enc_attn_ffn_split_kernel<4,2,1> enc_fuse_va_kernel<1,3> "
     "length_regulate_kernel max_i32_kernel" + _DEC),
    ("tiny", 2, 150, L150, 63, "encode",
     "enc_merge_qkv_kernel<4,1,3,1> attn_lds_kernel<8,32> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> enc_merge_qkv_kernel<1,2,1,2> enc_attn_ffn_split_kernel<4,2,1> enc_fuse_va_kernel<1,3> "
     "length_regulate_kernel max_i32_kernel"),
    ("tiny", 2, 150, L150, 31, "encode",
     "enc_merge_qkv_kernel<4,1,3,1> attn_lds_kernel<8,32> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> enc_merge_qkv_kernel<1,2,1,2> enc_attn_ffn_split_kernel<4,2,1> enc_fuse_va_kernel<1,3> "
     "length_regulate_kernel max_i32_kernel"),
    ("tiny", 1, 270, None, 63, "encode",
     "enc_merge_qkv_kernel<4,1,3,1> attn_long_kernel<1> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> enc_merge_qkv_kernel<1,2,1,2> attn_lds_kernel<8,64> convgemm_kernel<2,false> "
     "convgemm_kernel<1,false> convgemm_kernel<2,false> enc_fuse_va_kernel<1,3> length_regulate_kernel max_i32_kernel"),
    ("tiny", 2, 40, L40, 63, "block",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> attn_kernel<2> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> pool_mask_kernel attn_kernel<1> convgemm_kernel<2,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<2,false>"),
    ("tiny_e2", 2, 40, L40, 63, "forward",
     "enc_merge_qkv_kernel<4,1,3,1> attn_kernel<2> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> enc_merge_qkv_kernel<1,2,1,2> pool_mask_kernel attn_kernel<1> convgemm_kernel<2,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_kernel<2,false> enc_va16_kernel<3> max_i32_kernel" + _DEC),
    ("tiny_e2", 2, 40, L40, 63, "encode",
     "enc_merge_qkv_kernel<4,1,3,1> attn_kernel<2> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> enc_merge_qkv_kernel<1,2,1,2> pool_mask_kernel attn_kernel<1> convgemm_kernel<2,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_kernel<2,false> enc_va16_kernel<3> max_i32_kernel"),
    ("small", 2, 40, L40, 63, "forward",
     "enc_attn_ffn_kernel<2,2,1,4,3,1> enc_merge_qkv_kernel<2,4,1,2> enc_attn_ffn_kernel<2,4,1> enc_va64_kernel<1> "
     "max_i32_kernel" + _DEC),
    ("small", 2, 40, L40, 63, "encode",
     "enc_attn_ffn_kernel<2,2,1,4,3,1> enc_merge_qkv_kernel<2,4,1,2> enc_attn_ffn_kernel<2,4,1> enc_va64_kernel<1> "
     "max_i32_kernel"),
    ("small", 2, 150, L150, 63, "forward",
     "enc_merge_qkv_kernel<4,2,3,1> attn_lds_kernel<8,64> enc_post_attn64_kernel<2> enc_merge_qkv_kernel<2,4,1,2> "
     "enc_attn_ffn_kernel<4,4,1> enc_va64_kernel<2> max_i32_kernel" + _DEC),
    ("small", 2, 150, L150, 63, "encode",
     "enc_merge_qkv_kernel<4,2,3,1> attn_lds_kernel<8,64> enc_post_attn64_kernel<2> enc_merge_qkv_kernel<2,4,1,2> "
     "enc_attn_ffn_kernel<4,4,1> enc_va64_kernel<2> max_i32_kernel"),
    ("small", 2, 40, L40, 31, "forward",
     "enc_attn_ffn_kernel<2,2,1,4,3,1> enc_merge_qkv_kernel<2,4,1,2> enc_attn_ffn_kernel<2,4,1> enc_fuse_va_kernel<2,3> "
     "convgemm_dma_kernel<8,1,NWV,false,true> max_i32_kernel" + _DEC),
    ("small", 2, 40, L40, 0, "forward",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> attn_kernel<2> convgemm_kernel<2,false> "
     "convgemm_kernel<1,false> convgemm_kernel<2,false> convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> "
     "pool_mask_kernel attn_kernel<1> convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<1,false> "
     "convgemm_kernel<1,false> convgemm_kernel<2,false> convgemm_kernel<2,false> convgemm_kernel<2,false> "
     "convgemm_kernel<2,false> convgemm_kernel<2,false> convgemm_kernel<2,false> va_tail_kernel length_regulate_kernel "
     "convgemm_dma_kernel<8,1,NWV,false,true> max_i32_kernel" + _DEC),
    ("small", 2, 40, L40, 63, "block",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> attn_kernel<2> convgemm_kernel<2,false> "
     "convgemm_kernel<1,false> convgemm_kernel<1,false> convgemm_kernel<2,false> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> pool_mask_kernel attn_kernel<1> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true>"),
    ("base", 2, 40, L40, 63, "forward",
     "enc_merge_qkv_kernel<4,4,5,1> enc_attn_ffn_kernel<2,4,2> enc_merge_q256_kernel<3,4> pool_mask_kernel attn_kernel<1> "
     "convgemm_dma_kernel<8,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<8,1,NWV,false,true> enc_fuse128_kernel<5> enc_pred128_kernel "
     "convgemm_dma_kernel<8,1,NWV,false,true> max_i32_kernel" + _DEC),
    ("base", 2, 40, L40, 63, "encode",
     "enc_merge_qkv_kernel<4,4,5,1> enc_attn_ffn_kernel<2,4,2> enc_merge_q256_kernel<3,4> pool_mask_kernel attn_kernel<1> "
     "convgemm_dma_kernel<8,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<8,1,NWV,false,true> enc_fuse128_kernel<5> enc_pred128_kernel max_i32_kernel"),
    ("base", 2, 40, L40, 63, "encode_no_ln2",
     "enc_merge_qkv_kernel<4,4,5,1> enc_attn_ffn_kernel<2,4,2> enc_merge_q256_kernel<3,4> pool_mask_kernel attn_kernel<1> "
     "convgemm_dma_kernel<8,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<8,1,NWV,false,true> "
     "enc_fuse128_kernel<5> convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> va_tail_kernel length_regulate_kernel max_i32_kernel"),
    ("base", 2, 150, L150, 63, "encode",
     "enc_merge_qkv_kernel<4,4,5,1> attn_lds_kernel<8,128> enc_post_attn128_kernel enc_merge_q256_kernel<3,4> "
     "pool_mask_kernel attn_lds_kernel<4,128> convgemm_dma_kernel<8,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<8,1,NWV,false,true> enc_fuse128_kernel<5> "
     "enc_pred128_kernel max_i32_kernel"),
    ("base", 2, 40, L40, 31, "forward",
     "enc_merge_qkv_kernel<4,4,5,1> enc_attn_ffn_kernel<2,4,2> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> pool_mask_kernel attn_kernel<1> convgemm_dma_kernel<8,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<8,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> va_tail_kernel length_regulate_kernel convgemm_dma_kernel<8,1,NWV,false,true> "
     "max_i32_kernel" + _DEC),
    ("base", 2, 40, L40, 7, "encode",
     "enc_merge_qkv_kernel<4,4,5,1> enc_attn_ffn_kernel<2,4,2> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> pool_mask_kernel attn_kernel<1> convgemm_dma_kernel<8,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<8,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> va_tail_kernel length_regulate_kernel max_i32_kernel"),
    ("base", 2, 40, L40, 0, "forward",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> attn_kernel<2> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> "
     "pool_mask_kernel attn_kernel<1> convgemm_dma_kernel<8,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<8,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> va_tail_kernel length_regulate_kernel "
     "convgemm_dma_kernel<8,1,NWV,false,true> max_i32_kernel" + _DEC),
    ("base", 2, 40, L40, 63, "block",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> attn_kernel<2> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> enc_merge_q256_kernel<3,4> "
     "pool_mask_kernel attn_kernel<1> convgemm_dma_kernel<8,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<8,1,NWV,false,true>"),
    ("base_k3", 2, 71, [71, 38], 63, "forward",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> enc_attn_ffn_kernel<4,4,2> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> pool_mask_kernel attn_kernel<2> convgemm_dma_kernel<8,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<8,1,NWV,false,true> enc_fuse128_kernel<3> "
     "enc_pred128_kernel convgemm_dma_kernel<8,1,NWV,false,true> max_i32_kernel" + _DEC),
    ("base_k3", 2, 71, [71, 38], 63, "encode",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> enc_attn_ffn_kernel<4,4,2> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> pool_mask_kernel attn_kernel<2> convgemm_dma_kernel<8,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<8,1,NWV,false,true> enc_fuse128_kernel<3> "
     "enc_pred128_kernel max_i32_kernel"),
    ("base_k3", 2, 71, [71, 38], 31, "encode",
     "convgemm_kernel<1,false> convgemm_dma_kernel<4,1,NWV,false,true> enc_attn_ffn_kernel<4,4,2> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> pool_mask_kernel attn_kernel<2> convgemm_dma_kernel<8,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<8,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> convgemm_kernel<1,false> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> convgemm_dma_kernel<4,1,NWV,false,true> "
     "convgemm_dma_kernel<4,1,NWV,false,true> va_tail_kernel length_regulate_kernel max_i32_kernel"),
]


def _net(name):
    if name not in _NETS:
        sd = synth_state_dict(_CONFIGS[name], 1234)
        net = build_phoneme2mel(_CONFIGS[name])
        load_numpy_state_dict(net, sd)
        _NETS[name] = net, sd
    return _NETS[name]


def _without_ln2(predictors):
    """net.encoder._predictors with pitch / energy's ln2_g / ln2_b NULL"""
    def get(lib, stream):
        out = []
        for q, (w, keep) in enumerate(predictors(lib, stream)):
            w2 = _lib.PredictorWeights()
            ctypes.pointer(w2)[0] = w
            if q < 2:
                w2.ln2_g = w2.ln2_b = None
            out.append((w2, keep))
        return out
    return get


def run_entry(name, B, T, lens, plan, entry, full_records=False):
    """the kernels `entry` launches on the simulator (weight preparation left out), and its outputs.  full_records: each kernel as
    `name[gx,gy,gz|bx,by,bz|lds]`, with its grid, block and dynamic LDS bytes."""
    net, _ = _net(name)
    ids, mask = synth_phonemes(B, T, 5, lens)
    x = {"phoneme": torch.from_numpy(ids)}
    if B > 1:
        x["phoneme_mask"] = torch.from_numpy(mask)
    enc = net.encoder.encoder
    with use_sim(), torch.no_grad(), _lib.launch_plan(plan):
        if entry == "block":
            os.environ["ESMI_FOLD_FFN"] = "0"
            enc._cache.invalidate()
        try:
            with launch_records() as records:
                if entry == "forward":
                    out = net(x)
                elif entry == "encode":
                    out = net.encoder._encode(x)
                elif entry == "encode_no_ln2":
                    net.encoder._predictors = _without_ln2(type(net.encoder)._predictors.__get__(net.encoder))
                    try:
                        out = net.encoder._encode(x)
                    finally:
                        del net.encoder._predictors
                else:
                    out = enc(x["phoneme"], mask=x.get("phoneme_mask"))
        finally:
            if entry == "block":
                os.environ.pop("ESMI_FOLD_FFN", None)
                enc._cache.invalidate()
    return " ".join(f"{n}[{dims}]" if full_records else n for n, dims in records if not n.startswith(_PREP)), out


@pytest.mark.parametrize("name,B,T,lens,plan,entry,expected", ROWS, ids=[f"{r[0]}-B{r[1]}-T{r[2]}-plan{r[4]}-{r[5]}" for r in ROWS])
def test_dispatch_launches(name, B, T, lens, plan, entry, expected):
    got, out = run_entry(name, B, T, lens, plan, entry)
    assert got == expected
    if entry == "encode_no_ln2":   # the per-op predictors never read the NULL weights: the oracle's values
        _, sd = _net(name)
        ids, mask = synth_phonemes(B, T, 5, lens)
        o = oracle.phoneme2mel(_CONFIGS[name], oracle.Weights(sd), ids, mask)
        for key in ("pitch", "energy", "duration"):
            np.testing.assert_allclose(out[key].numpy(), getattr(o, key), atol=H.PRED_TOL, rtol=0, err_msg=key)


# The names above do not tell a convolution from another of the same kernel.  One row of the one-kernel-per-op plan with the complete
# records -- grid, block, dynamic LDS bytes per launch -- so that a descriptor with a wrong c_out, n_out or ldo, which changes a grid, is
# seen: tiny ES, B = 2, T = 40, plan 0, the one-call forward (both blocks, Fuse, the predictors, the decoder head's GEMM).
PER_OP_RECORDS = (
    "convgemm_kernel<1,false>[1,1,1|256,1,1|0] convgemm_dma_kernel<4,1,NWV,false,true>[8,1,1|256,1,1|49152] "
    "attn_kernel<2>[1,1,1|256,1,1|0] convgemm_kernel<1,false>[1,1,1|256,1,1|0] convgemm_kernel<1,false>[1,1,1|256,1,1|0] "
    "convgemm_kernel<1,false>[1,1,1|256,1,1|0] convgemm_kernel<1,false>[1,2,1|256,1,1|0] "
    "convgemm_dma_kernel<4,1,NWV,false,true>[8,1,1|256,1,1|49152] pool_mask_kernel[1,1,1|256,1,1|0] "
    "attn_kernel<1>[1,1,1|256,1,1|0] convgemm_kernel<2,false>[1,1,1|256,1,1|0] convgemm_kernel<1,false>[1,2,1|256,1,1|0] "
    "convgemm_kernel<2,false>[1,1,1|256,1,1|0] convgemm_kernel<1,false>[1,1,1|256,1,1|0] "
    "convgemm_kernel<1,false>[1,1,1|256,1,1|0] convgemm_kernel<1,false>[1,1,1|256,1,1|0] "
    "convgemm_kernel<1,false>[1,1,1|256,1,1|0] convgemm_kernel<1,false>[1,1,1|256,1,1|0] "
    "convgemm_kernel<1,false>[1,1,1|256,1,1|0] convgemm_kernel<1,false>[1,1,1|256,1,1|0] "
    "convgemm_kernel<1,false>[1,1,1|256,1,1|0] convgemm_kernel<1,false>[1,1,1|256,1,1|0] "
    "convgemm_kernel<1,false>[1,1,1|256,1,1|0] va_tail_kernel[3,1,1|256,1,1|0] length_regulate_kernel[2,1,1|64,1,1|0] "
    "convgemm_dma_kernel<4,1,NWV,false,true>[8,1,1|256,1,1|49152] max_i32_kernel[1,1,1|64,1,1|0] "
    "mel_decoder_kernel<DX2,KD,NW>[16,1,1|512,1,1|75840] "
)


def test_per_op_plan_launch_records():
    got, _ = run_entry("tiny", 2, 40, L40, 0, "forward", full_records=True)
    assert got.split() == PER_OP_RECORDS.split()


if __name__ == "__main__":   # prints PER_OP_RECORDS, to re-record after an intended change of the launches
    import textwrap
    for ln in textwrap.wrap(run_entry("tiny", 2, 40, L40, 0, "forward", full_records=True)[0], 116, break_long_words=False, break_on_hyphens=False):
        print(f'    "{ln} "')
