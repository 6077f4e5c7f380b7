"""The training step at bf16-mixed precision: `TrainStep(precision="bf16")`, `esmi_conv_desc.precision = ESMI_PRECISION_BF16`.

The forward and data-gradient GEMMs of every dense convolution / Linear / ConvTranspose1d round both operands to bfloat16 (nearest
even) and run one v_mfma_f32_32x32x16_bf16 per 16 channels -- `convgemm_bf16_kernel`, `convgemm_dma_bf16_kernel`,
`pwgemm_bf16_kernel` --; nothing is scaled, there is no loss scaler, no max|dy| pass and no skipped step.  The check bodies
(tests/train_bf16_checks.py) run on the wave simulator here (its family thresholds are 1 row) and on the device under `-m gpu` at
the smallest shapes that reach each kernel there (`pwgemm` from 32,768 rows, `convgemm_dma` from 2,048, MT = 2 from ~131,000)."""
import os
import re
import subprocess
import sys

import pytest

from tests import train_bf16_checks as K
from tests.test_train_gemm_at_size import OTHER_FAMILIES

gpu = pytest.mark.gpu
_nowarn = pytest.mark.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- 1. operator level, the simulator
SIM_CONVS = [   # tests/test_train_gemm_at_size.SIM_AMP_CONVS' shapes -> the bf16 kernels they must launch
    ((128, 128, 1, 1, 0, False, 1, 70), "128to128", ("pwgemm_bf16_kernel<8,2>",)),
    ((128, 80, 1, 1, 0, False, 2, 45), "128to80", ("pwgemm_bf16_kernel<8,2>", "pwgemm_bf16_kernel<5,2>")),
    ((128, 128, 3, 1, 1, False, 2, 37), "dma_k3", ("convgemm_dma_bf16_kernel<4,1,NWV>",)),
    ((32, 32, 3, 1, 1, False, 2, 37), "cin32_k3", ("convgemm_bf16_kernel<1>",)),
    ((32, 64, 3, 2, 1, False, 2, 19), "stride2_odd", ("convgemm_bf16_kernel<1>",)),
    ((64, 32, 3, 2, 0, True, 2, 9), "convT_crop", ("convgemm_bf16_kernel<1>",)),
    ((40, 24, 3, 1, 1, False, 1, 11), "cin40", ("convgemm_bf16_kernel<1>",)),
]
F16_OR_FP32_GEMM = re.compile(r"^(convgemm_kernel<|convgemm_dma_kernel<|pwgemm_kernel<|convgemm_len)")


def _no_other_gemm(names):
    other = sorted({n for n in names if F16_OR_FP32_GEMM.match(n)} | {n for n in names if n == "absmax_kernel"})
    assert not other, other


@_nowarn
@pytest.mark.parametrize("cfg,expect", [(c, e) for c, _, e in SIM_CONVS], ids=[i for _, i, _ in SIM_CONVS])
def test_simulated_conv_matches_rounded_operand_model(cfg, expect):
    with K.on_sim(expect) as names:
        K.check_conv(cfg)
    _no_other_gemm(names)


@_nowarn
@pytest.mark.parametrize("cin,cout,variant,expect", [
    (128, 128, "tanh", "pwgemm_bf16_kernel<8,4>"), (128, 128, "res_mask", "pwgemm_bf16_kernel<8,4>"),
    (128, 128, "relu_out_mask", "pwgemm_bf16_kernel<8,4>"), (80, 128, "res_mask", "pwgemm_bf16_kernel<5,4>"),
    # 256 channels (the dim = 256 decoder's layer): the fused conv + LayerNorm launch stops at 128, so the Linear runs on its own -- two
    # 128-column tiles of the LDS-staged kernel -- and the norm as a second launch
    (256, 256, "tanh", "convgemm_dma_bf16_kernel<4,1,NWV>")])
def test_simulated_layernorm_epilogue_variants(cin, cout, variant, expect):
    with K.on_sim((expect,)) as names:
        K.check_conv_ln(cin, cout, 2, 35, variant)
    _no_other_gemm(names)


@_nowarn
def test_simulated_ragged_last_tile_writes_nothing_past_the_end():
    with K.on_sim(("pwgemm_bf16_kernel<8,2>", "pwgemm_bf16_kernel<5,4>")) as names:
        K.check_ragged_tile_stays_in_bounds(128, 80, 1, 33, False)
        K.check_ragged_tile_stays_in_bounds(80, 128, 1, 33, True)
    _no_other_gemm(names)


# --------------------------------------------------------------------------------------------- 1. operator level, the device
PW_ROWS = [(4, 8192), (1, 32768 + 33)]       # the 32,768-row threshold exactly; the ragged last tile


@gpu
@pytest.mark.parametrize("rows", PW_ROWS, ids=["rows32768", "rows32801"])
@pytest.mark.parametrize("cout", [128, 80])
def test_gpu_pwgemm_linear(cout, rows):
    """128 -> 128: `pwgemm_bf16_kernel<8, 2>` both ways; 128 -> 80: the data gradient is `<5, 2>`."""
    K.check_conv((128, cout, 1, 1, 0, False) + rows)


@gpu
@pytest.mark.parametrize("rows", PW_ROWS, ids=["rows32768", "rows32801"])
@pytest.mark.parametrize("cin,variant", [(128, "tanh"), (128, "res_mask"), (128, "relu_out_mask"), (80, "res_mask")])
def test_gpu_pwgemm_layernorm_epilogue(cin, variant, rows):
    """`pwgemm_bf16_kernel<8, 4>` / `<5, 4>` with the LayerNorm epilogue."""
    K.check_conv_ln(cin, 128, *rows, variant)


@gpu
@pytest.mark.parametrize("cin,cout,ln", [(128, 128, False), (128, 80, False), (128, 128, True), (80, 128, True)],
                         ids=["128to128", "128to80", "128to128_ln", "80to128_ln"])
def test_gpu_pwgemm_ragged_last_tile_writes_nothing_past_the_end(cin, cout, ln):
    K.check_ragged_tile_stays_in_bounds(cin, cout, 1, 32768 + 33, ln)


_FAMILY = dict((i, c) for c, i in OTHER_FAMILIES)


@gpu
@pytest.mark.parametrize("case", ["dma_k3_mt1", "dma_k3_mt2", "stride2_odd_nt1", "convT_crop_nt1", "cin40_nt1", "stride2_odd_nt2",
                                  "stride2_odd_nt4", "convT_crop_nt4"])
def test_gpu_dma_and_streaming_families(case):
    """`convgemm_dma_bf16_kernel<4, 1>` (2,400 rows), `<4, 2>` (131,072 rows), `convgemm_bf16_kernel<1 | 2 | 4>`, MODE_CONV and MODE_CONVT."""
    K.check_conv(_FAMILY[case])


@gpu
def test_gpu_256_channel_layernorm_layer():
    """256 -> 256 + tanh + LayerNorm at 2,400 rows: `convgemm_dma_bf16_kernel<4, 1>` over two column tiles, then the norm."""
    K.check_conv_ln(256, 256, 4, 600, "tanh")


# -------------------------------------------------------------------------------------------------------- 2. the rounding is RNE
SIM_RNE = [((128, 128, 1, 1, 0, False, 1, 70), "pwgemm"), ((128, 128, 3, 1, 1, False, 2, 37), "dma"), ((32, 64, 3, 2, 1, False, 2, 19), "streaming")]
GPU_RNE = [((128, 128, 1, 1, 0, False, 4, 8192), "pwgemm"), ((128, 128, 3, 1, 1, False, 4, 600), "dma"), ((128, 128, 3, 2, 1, False, 4, 131), "streaming")]


@_nowarn
@pytest.mark.parametrize("cfg", [c for c, _ in SIM_RNE], ids=[i for _, i in SIM_RNE])
def test_simulated_rounding_is_nearest_even_and_nothing_else_rounds(cfg):
    with K.on_sim():
        K.check_rounding_is_rne(cfg)


@gpu
@pytest.mark.parametrize("cfg", [c for c, _ in GPU_RNE], ids=[i for _, i in GPU_RNE])
def test_gpu_rounding_is_nearest_even_and_nothing_else_rounds(cfg):
    K.check_rounding_is_rne(cfg)


# ------------------------------------------------------------------------------------- 3. one step against the reference's bf16 run
def test_bf16_fixture_is_a_bf16_run():
    import numpy as np
    g = np.load(K.GOLD_BF16)
    assert str(g["out_dtype"]) == "torch.bfloat16" and not any(k.startswith("after.") for k in g.files)
    assert sum(k.startswith("grad.") for k in g.files) >= 60


@_nowarn
def test_simulated_step_matches_reference_bf16():
    """(the figures of this run and of the device's: profiles/r14_train_bf16.md)"""
    with K.on_sim():
        K.check_step_against_reference("cpu")


@gpu
def test_gpu_step_matches_reference_bf16():
    K.check_step_against_reference("cuda")


# ------------------------------------------------------------------------------------------------------------------ 4. mechanics
@_nowarn
def test_simulated_mechanics():
    with K.on_sim():
        K.check_mechanics("cpu")


@gpu
def test_gpu_mechanics():
    K.check_mechanics("cuda")


@_nowarn
def test_simulated_inference_sees_the_update():
    with K.on_sim():
        K.check_inference_sees_the_update("cpu", 2)


@gpu
def test_gpu_training_reduces_the_loss_and_inference_sees_the_update():
    first, last = K.check_inference_sees_the_update("cuda", 21)
    assert last < 0.9 * first, (first, last)


@_nowarn
def test_simulated_abi_refuses_other_precisions():
    with K.on_sim() as names:
        K.check_abi_refuses_other_precisions("cpu")
    assert not names, names          # nothing launched


@gpu
def test_gpu_abi_refuses_other_precisions():
    K.check_abi_refuses_other_precisions("cuda")


@gpu
def test_gpu_captured_step_equals_eager_step():
    """graph=True captures a bf16 step like any other: tests/test_train_step.test_gpu_captured_step_equals_eager_step's tolerances."""
    import torch
    from tests.test_train_step import _setup
    train, g, net, x, y = _setup("cuda", K.GOLD_BF16)
    eager = train.TrainStep(net, lr=1e-3, precision="bf16")
    ref = [eager.step(x, y).clone() for _ in range(4)]
    t2, g2, net2, x2, y2 = _setup("cuda", K.GOLD_BF16)
    cap = t2.TrainStep(net2, lr=1e-3, graph=True, precision="bf16")
    got = [cap.step(x2, y2).clone() for _ in range(4)]
    for a, b in zip(ref, got):
        assert torch.allclose(a, b, rtol=1e-5, atol=0), (a, b)
    assert torch.allclose(eager.flat.data, cap.flat.data, rtol=1e-4, atol=1e-6)
    assert cap.t == 4 and cap.skipped == 0 and cap.scale == 1.0


# ------------------------------------------------------------------------------------------------------------------- 5. launches
def _bf16_step():
    from tests.test_train_step import _setup
    train, _, net, x, y = _setup("cpu", K.GOLD_BF16)
    return lambda: train.TrainStep(net, precision="bf16").step(x, y)


def _f16_step():
    from tests.test_train_step import _setup
    train, _, net, x, y = _setup("cpu", K.GOLD_BF16)
    return lambda: train.TrainStep(net, precision=16).step(x, y)


BF16_STEP = (195, "c88a2e1f02f7dc97",
             "train_pack_batch_kernel train_embed_fwd_kernel convgemm_dma_bf16_kernel<4,1,NWV> convgemm_bf16_kernel<1> "
             "convgemm_dma_bf16_kernel<4,1,NWV> train_attn_fwd_lds_kernel convgemm_bf16_kernel<1> train_ln_fwd4_kernel<8> 2x "
             "convgemm_bf16_kernel<1> train_act_fwd_kernel convgemm_bf16_kernel<1> train_ln_fwd4_kernel<8> 2x "
             "convgemm_bf16_kernel<1> pool_mask_kernel convgemm_dma_bf16_kernel<4,1,NWV> train_attn_fwd_lds_kernel "
             "convgemm_bf16_kernel<1> train_ln_fwd4_kernel<16> 2x convgemm_bf16_kernel<1> train_act_fwd_kernel "
             "convgemm_bf16_kernel<1> train_ln_fwd4_kernel<16> 3x convgemm_bf16_kernel<1> train_cat_kernel convgemm_bf16_kernel<1> "
             "train_mask_rows_kernel convgemm_bf16_kernel<1> train_ln_fwd4_kernel<8> convgemm_bf16_kernel<1> conv_to1_kernel "
             "convgemm_bf16_kernel<1> train_ln_fwd4_kernel<8> convgemm_bf16_kernel<1> conv_to1_kernel convgemm_bf16_kernel<1> "
             "train_ln_fwd4_kernel<8> convgemm_bf16_kernel<1> conv_to1_kernel train_ln_fwd4_kernel<8> bucket_embed_kernel "
             "train_embed_fwd_kernel bucket_embed_kernel train_embed_fwd_kernel train_cat_kernel length_regulate_kernel "
             "train_repeat_fwd4_kernel pwgemm_bf16_kernel<8,2> train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_bf16_kernel<8,2> "
             "train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_bf16_kernel<8,2> 2x train_ln_fwd4_kernel<32> train_conv_dw_kernel "
             "pwgemm_bf16_kernel<8,2> train_ln_fwd4_kernel<32> train_conv_dw_kernel pwgemm_bf16_kernel<8,2> 2x "
             "train_ln_fwd4_kernel<32> pwgemm_bf16_kernel<8,2> train_loss_partial_kernel train_loss_final_kernel "
             "train_loss_grad_kernel train_conv_wgrad_mfma_kernel<false> pwgemm_bf16_kernel<5,2> 2x train_ln_bwd4_kernel<32> "
             "train_conv_wgrad_mfma_kernel<false> pwgemm_bf16_kernel<8,2> train_conv_dw_kernel train_conv_wgrad_dw4_kernel "
             "train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_bf16_kernel<8,2> train_conv_dw_kernel "
             "train_conv_wgrad_dw4_kernel 2x train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> pwgemm_bf16_kernel<8,2> "
             "train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> train_conv_wgrad_mfma_kernel<false> "
             "pwgemm_bf16_kernel<8,2> train_conv_dw_kernel train_conv_wgrad_dw4_kernel train_ln_bwd4_kernel<32> "
             "train_conv_wgrad_mfma_kernel<false> pwgemm_bf16_kernel<8,2> train_repeat_bwd_kernel train_cat_kernel 2x "
             "train_embed_bwd_kernel train_ln_bwd4_kernel<8> train_act_bwd_kernel train_lin1_bwd4_kernel<8> train_act_bwd_kernel "
             "convgemm_bf16_kernel<1> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<8> convgemm_bf16_kernel<1> "
             "train_conv_wgrad_kernel train_colsum_kernel train_lin1_bwd4_kernel<8> train_act_bwd_kernel convgemm_bf16_kernel<1> "
             "train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<8> convgemm_bf16_kernel<1> train_conv_wgrad_kernel "
             "train_colsum_kernel train_lin1_bwd4_kernel<8> train_act_bwd_kernel convgemm_bf16_kernel<1> train_conv_wgrad_kernel "
             "train_colsum_kernel train_ln_bwd4_kernel<8> convgemm_bf16_kernel<1> train_conv_wgrad_kernel train_colsum_kernel "
             "train_mask_rows_kernel convgemm_bf16_kernel<1> train_conv_wgrad_kernel train_colsum_kernel train_cat_kernel "
             "convgemm_bf16_kernel<1> train_conv_wgrad_kernel train_colsum_kernel convgemm_bf16_kernel<1> train_conv_wgrad_kernel "
             "train_colsum_kernel convgemm_bf16_kernel<1> train_conv_wgrad_kernel train_colsum_kernel train_ln_bwd4_kernel<16> "
             "convgemm_bf16_kernel<1> train_conv_wgrad_kernel train_colsum_kernel train_act_bwd_kernel convgemm_bf16_kernel<1> "
             "train_conv_wgrad_kernel train_colsum_kernel convgemm_bf16_kernel<1> train_conv_wgrad_kernel train_colsum_kernel "
             "train_ln_bwd4_kernel<16> convgemm_dma_bf16_kernel<4,1,NWV> train_conv_wgrad_kernel train_colsum_kernel "
             "train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel convgemm_bf16_kernel<1> train_conv_wgrad_kernel "
             "convgemm_bf16_kernel<1> train_conv_wgrad_kernel convgemm_bf16_kernel<1> train_conv_wgrad_kernel "
             "train_ln_bwd4_kernel<8> convgemm_bf16_kernel<1> train_conv_wgrad_kernel train_colsum_kernel train_act_bwd_kernel "
             "convgemm_bf16_kernel<1> train_conv_wgrad_kernel train_colsum_kernel convgemm_bf16_kernel<1> train_conv_wgrad_kernel "
             "train_colsum_kernel train_reduce_batch_kernel train_ln_bwd4_kernel<8> convgemm_bf16_kernel<1> train_conv_wgrad_kernel "
             "train_colsum_kernel train_attn_bwd_rows_lds_kernel train_attn_bwd_cols_kernel convgemm_bf16_kernel<1> "
             "train_conv_wgrad_kernel convgemm_dma_bf16_kernel<4,1,NWV> train_conv_wgrad_kernel convgemm_dma_bf16_kernel<4,1,NWV> "
             "train_conv_wgrad_kernel train_embed_bwd_kernel train_reduce_batch_kernel train_adamw_kernel ")


def test_bf16_step_launches():
    """One bf16 step on the simulator: no binary16-AMP or fp32-accurate instantiation of the three GEMM families, no absmax kernel
    (neither the data gradients' max|dy| nor the scaler's max|g| over the flat gradient), and otherwise precision 16's launches name
    for name; kernel names, grids, blocks and LDS sizes pinned as tests/test_train_dispatch.py pins its rows
    (`python -m tests.test_train_bf16` prints the row)."""
    from tests.test_train_dispatch import launch_log, summarize
    count, digest, text = summarize(launch_log(_bf16_step))
    names = text.split()
    _no_other_gemm(names)
    assert not [n for n in names if "absmax" in n], names
    f16_count, _, f16_text = summarize(launch_log(_f16_step))
    twin = {"convgemm_kernel<1,true>": "convgemm_bf16_kernel<1>", "convgemm_dma_kernel<4,1,NWV,true,false>": "convgemm_dma_bf16_kernel<4,1,NWV>",
            "pwgemm_kernel<8,2,true>": "pwgemm_bf16_kernel<8,2>", "pwgemm_kernel<5,2,true>": "pwgemm_bf16_kernel<5,2>"}
    want = " ".join(twin.get(n, n) for n in f16_text.split())
    want = re.sub(r"(\d+x )?absmax_kernel ", "", want).replace("train_bump_step_kernel train_adamw_dev_kernel", "train_adamw_kernel")
    # (run lengths next to a removed absmax launch merge: compare the expanded sequences)
    assert _expand(text) == _expand(want)
    assert count < f16_count
    assert (count, digest) == BF16_STEP[:2] and names == BF16_STEP[2].split()


def _expand(text):
    out, k = [], 1
    for tok in text.split():
        m = re.fullmatch(r"(\d+)x", tok)
        if m:
            k = int(m.group(1))
        else:
            out += [tok] * k
            k = 1
    return out


# ------------------------------------------------------------------------------------------------------------------ 6. resources
LIB = os.path.join(ROOT, "efficientspeech_amd", "libesmi.so")


def test_bf16_kernels_spill_no_more_than_their_f16_twins():
    """From tools/kernel_resources.py --all (no GPU): every bf16 instantiation exists and has no more scratch than its binary16 twin --
    0 B where tests/test_kernel_resources.py pins the twin at 0, at most 64 B for the NT = 4 pwgemm and NT = 8 dma shapes."""
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), LIB, "--all"], capture_output=True, text=True, check=True).stdout
    rows = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\| `(.+?)` \| [^|]+ \| (\d+) \|", out, re.M)}
    twins = {}
    for nt in (1, 2, 4, 8):
        twins[f"convgemm_bf16_kernel<{nt}>"] = (f"convgemm_kernel<{nt}, true>", 0 if nt <= 4 else None)
    for nt, mt in ((4, 1), (4, 2), (8, 1)):
        twins[f"convgemm_dma_bf16_kernel<{nt}, {mt}, 4>"] = (f"convgemm_dma_kernel<{nt}, {mt}, 4, true, false>", 0 if nt == 4 else 64)
    for ks, nt in ((8, 2), (8, 4), (5, 2), (5, 4)):
        twins[f"pwgemm_bf16_kernel<{ks}, {nt}>"] = (f"pwgemm_kernel<{ks}, {nt}, true>", 0 if nt == 2 else 64)
    assert sorted(k for k in rows if "bf16_kernel" in k and "gemm" in k) == sorted(twins), sorted(k for k in rows if "bf16_kernel" in k)
    for mine, (twin, cap) in twins.items():
        assert rows[mine] <= rows[twin], (mine, rows[mine], twin, rows[twin])
        assert cap is None or rows[mine] <= cap, (mine, rows[mine], cap)


if __name__ == "__main__":
    import textwrap
    from tests.test_train_dispatch import launch_log, summarize
    os.environ.setdefault("WAVESIM_THREADS", "16")
    count, digest, text = summarize(launch_log(_bf16_step))
    lines = textwrap.wrap(text, 118, break_long_words=False, break_on_hyphens=False)
    print(f'BF16_STEP = ({count}, "{digest}",')
    print("\n".join(f'             "{ln} "' for ln in lines) + ")")
