"""The variance adaptor's discrete decisions at exact ties, in every kernel that makes them: torch.bucketize(right=False) as spelt by
bucket_count_lds<2> (enc_va16, enc_all16), <4> (enc_va64), <8> (enc_pred128, INFINITY in the 128th slot), the register-resident edges of
enc_fuse_va (DIM 32 / 64), the binary search of va_tail and bucket_embed_kernel; torch.round as spelt by va_duration and by enc_fuse_va.
Values sit ON an edge and one fp32 step beside it, duration products ON a .5; the expectation is torch's own operators on the CPU and
every decision is compared bit for bit.  The checks live in tests/va_ties_checks.py; the CPU tier runs them through the wave simulator
(the same kernel sources compiled for the host) and asserts the kernel that decided, the GPU tier on the device (the same host code
dispatches there: tests/test_dispatch.py)."""
import pytest

from tests import va_ties_checks as V
from tests.simlib import launched_kernels, use_sim

DEV = "cuda:0"
# config, plan, shape, the kernel that decides (simulator: asserted from the launch log)
TEACHER = [("tiny", 63, V.TEACHER_SHAPES["tiny"], "enc_va16_kernel"),
           ("tiny", 31, V.TEACHER_SHAPES["tiny"], "enc_fuse_va_kernel"),
           ("tiny", 7, V.TEACHER_SHAPES["tiny"], "enc_fuse_va_kernel"),
           ("tiny", 0, V.TEACHER_SHAPES["tiny"], "va_tail_kernel"),
           ("tiny", 63, V.HALO_SHAPES["tiny"], "enc_fuse_va_kernel"),
           ("small", 63, V.TEACHER_SHAPES["small"], "enc_va64_kernel"),
           ("small", 31, V.TEACHER_SHAPES["small"], "enc_fuse_va_kernel"),
           ("small", 0, V.TEACHER_SHAPES["small"], "va_tail_kernel"),
           ("small", 63, V.HALO_SHAPES["small"], "enc_fuse_va_kernel"),
           ("base", 63, V.TEACHER_SHAPES["base"], "enc_pred128_kernel"),
           ("base", 31, V.TEACHER_SHAPES["base"], "va_tail_kernel")]
TEACHER_IDS = [f"{n}-{p}-T{s[1]}" for n, p, s, _ in TEACHER]
# the prediction route: config, plan, entry point, deciding kernel
PRED = [("tiny", 63, "forward", "enc_all16_kernel"), ("tiny", 63, "encode", "enc_va16_kernel"), ("tiny", 31, "encode", "enc_fuse_va_kernel"),
        ("tiny", 7, "encode", "enc_fuse_va_kernel"), ("tiny", 0, "encode", "va_tail_kernel"),
        ("small", 63, "forward", "enc_va64_kernel"), ("small", 63, "encode", "enc_va64_kernel"), ("small", 31, "encode", "enc_fuse_va_kernel"),
        ("small", 0, "encode", "va_tail_kernel"),
        ("base", 63, "forward", "enc_pred128_kernel"), ("base", 63, "encode", "enc_pred128_kernel"), ("base", 31, "encode", "va_tail_kernel")]
PRED_IDS = [f"{n}-{p}-{e}" for n, p, e, _ in PRED]


@pytest.fixture(scope="module", autouse=True)
def shared_runs():
    yield
    V.clear()


def _names(seen):
    return {k.split("<")[0] for k in seen}


# ---------------------------------------------------------------------------------------------------------------- CPU tier
# (base ES: the roll-0 pass only on the simulator, 8 - 12 s a call; both on the device)
SIM_TEACHER = [(c, r) for c in TEACHER for r in V.ROLLS if not (c[0] == "base" and r)]


@pytest.mark.parametrize("case,roll", SIM_TEACHER, ids=[f"{c[0]}-{c[1]}-T{c[2][1]}-roll{r}" for c, r in SIM_TEACHER])
def test_simulated_teacher_values_on_every_edge(case, roll):
    """1. V(bins) = every edge, its two fp32 neighbours, e_0 - 1, e_last + 1, +-inf, +-0, +-3e38, +-denormal through
    `_encode(x, train=True)`: pitch_idx / energy_idx are torch.bucketize's and the two embedding slices of `feat` are the table rows, bit
    for bit; padded rows are zero.  The list rolled by 0 and by 13 rows.  `<=` for `<` in bucket_count_lds, or in any other spelling,
    fails this on dim - 1 rows at least (asserted on the inputs)."""
    name, plan, shape, kernel = case
    with use_sim(), launched_kernels() as seen:
        V.check_teacher(name, plan, shape, roll, "cpu")
    assert kernel in _names(seen), sorted(_names(seen))


def _whole(c):
    """a simulated case cheap enough for one test: tiny ES, and small ES through `_encode` (2 s a call)"""
    return c[0] == "tiny" or (c[0] == "small" and c[2] == "encode")


@pytest.mark.parametrize("name,plan,entry,kernel", [c for c in PRED if _whole(c)], ids=[i for c, i in zip(PRED, PRED_IDS) if _whole(c)])
def test_simulated_predictions_on_every_edge_and_half(name, plan, entry, kernel):
    """2. The zero-Linear checkpoint (raw predictions == the biases 1, 1, .5 bit for bit: asserted first) under (B,) control tensors:
    pitch products on V(pitch_bins), energy products on V(energy_bins) reversed, duration products 0, .5, 1, ... 7.5, both sides of 2.5
    and 1.5, and -1.5; T = 5, lengths cycling 5, 3, 1, calls of 32 utterances.  Indices, rounded durations (half to even, masked, clamped),
    scan and mel_len bit for bit; the one-call forward's plain call gives the tapped call's mel; its first mel against the oracle
    teacher-forced on the same products.  roundf for rintf in va_duration fails this (asserted on the inputs: floor(x + .5) differs)."""
    with use_sim(), launched_kernels() as seen:
        V.check_predictions(name, plan, entry, "cpu", mel=True, decode=[-1])
    assert kernel in _names(seen), sorted(_names(seen))


CALLS = {"small": len(range(0, 3 * 63 + 10, V.PRED_CHUNK)), "base": len(range(0, 3 * 127 + 10, V.PRED_CHUNK))}
# (a simulated base ES call of 32 utterances costs 9 s: the one-call forward decides all 391 utterances, one call per test; `_encode`,
#  which reaches the same enc_pred128 through the other entry point, and va_tail, whose 127 edges the teacher route has covered, take
#  the first and the last call; the device runs every call of every row)
PER_CALL = [(c, k) for c in PRED if not _whole(c) for k in (range(CALLS[c[0]]) if c[2] == "forward" else (0, CALLS[c[0]] - 1))]


@pytest.mark.parametrize("case,call", PER_CALL, ids=[f"{c[0]}-{c[1]}-{c[2]}-call{k}" for c, k in PER_CALL])
def test_simulated_predictions_on_every_edge_and_half_per_call(case, call):
    """2. small ES's one-call forward (199 utterances) and base ES (391), one call of 32 utterances per test"""
    name, plan, entry, kernel = case
    assert CALLS[name] == len(V.prediction_case(name))
    with use_sim(), launched_kernels() as seen:
        V.check_predictions(name, plan, entry, "cpu", chunks=[call], mel=True, decode=[-1], plain=name != "base")
    assert kernel in _names(seen), sorted(_names(seen))


@pytest.mark.parametrize("name,plan,entry", [("tiny", 63, "forward"), ("tiny", 63, "encode"), ("tiny", 31, "encode"), ("tiny", 0, "encode"),
                                             ("small", 63, "forward"), ("base", 63, "encode")])
def test_simulated_single_utterance_is_not_clamped(name, plan, entry):
    """2. B == 1, no mask: scale 3 -> 2 frames per phoneme; scale -3 -> a stored duration of -2, scan 0, mel_len 0, mel (1, 0, 80)"""
    with use_sim():
        V.check_single_utterance(name, plan, entry, "cpu")


@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_simulated_bucket_embed_on_every_edge(name):
    """3. bucket_embed_kernel through AcousticDecoder.get_embedding and train._bucket_embedding (with the table's gradient)"""
    with use_sim(), launched_kernels() as seen:
        V.check_bucket_embed(name, "cpu")
        V.check_train_bucket_embed(name, "cpu")
    assert "bucket_embed_kernel" in _names(seen), sorted(_names(seen))


@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_oracle_decides_as_torch_does(name):
    """4. the C oracle, pinned the same way (no kernel of ours): an oracle that shared a kernel's mistake would vouch for it"""
    V.check_oracle_teacher(name)
    V.check_oracle_teacher(name, nan=True)
    if name == "tiny":
        V.check_oracle_rounding()


NAN_CASES = [("tiny", 63, "enc_va16_kernel"), ("tiny", 31, "enc_fuse_va_kernel"), ("tiny", 0, "va_tail_kernel"), ("small", 63, "enc_va64_kernel"),
             ("small", 31, "enc_fuse_va_kernel"), ("base", 63, "enc_pred128_kernel")]


@pytest.mark.parametrize("name,plan,kernel", NAN_CASES, ids=[f"{n}-{p}" for n, p, _ in NAN_CASES])
def test_simulated_nan_takes_bucket_zero(name, plan, kernel):
    """5. What the project does today: no edge is below a NaN, so a NaN teacher value, and a NaN product from a NaN `pitch_control` /
    `energy_control`, gets index 0 -- inside the table; the embedding slice is row 0 -- in every deciding kernel, where torch.bucketize
    gives dim - 1.  (NaN durations without a mask are left out: (int)NaN is not defined.)"""
    with use_sim(), launched_kernels() as seen:
        V.check_teacher(name, plan, V.NAN_SHAPE, 0, "cpu", nan=True)
        V.check_predictions(name, plan, "encode", "cpu", nan=True)
    assert kernel in _names(seen), sorted(_names(seen))


def test_simulated_nan_takes_bucket_zero_in_bucket_embed_and_the_one_call_forward():
    with use_sim(), launched_kernels() as seen:
        V.check_bucket_embed("tiny", "cpu", nan=True)
        V.check_train_bucket_embed("tiny", "cpu", nan=True)
        V.check_predictions("tiny", 63, "forward", "cpu", nan=True)
    assert {"bucket_embed_kernel", "enc_all16_kernel"} <= _names(seen), sorted(_names(seen))


# ---------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("roll", V.ROLLS)
@pytest.mark.parametrize("name,plan,shape,kernel", TEACHER, ids=TEACHER_IDS)
def test_teacher_values_on_every_edge(name, plan, shape, kernel, roll):
    V.check_teacher(name, plan, shape, roll, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["forward", "encode"])
@pytest.mark.parametrize("plan", [63, 31, 7, 0])
@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_predictions_on_every_edge_and_half(name, plan, entry):
    """2. on the device: every call of every config, both entry points under every plan, the decoder and the plain call each time"""
    V.check_predictions(name, plan, entry, DEV, mel=True)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["forward", "encode"])
@pytest.mark.parametrize("plan", [63, 31, 7, 0])
@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_single_utterance_is_not_clamped(name, plan, entry):
    V.check_single_utterance(name, plan, entry, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "small", "base"])
def test_bucket_embed_on_every_edge(name):
    V.check_bucket_embed(name, DEV)
    V.check_train_bucket_embed(name, DEV)
    V.check_bucket_embed(name, DEV, nan=True)
    V.check_train_bucket_embed(name, DEV, nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,plan,shape,kernel", TEACHER, ids=TEACHER_IDS)
def test_nan_takes_bucket_zero(name, plan, shape, kernel):
    """5. on the device: the teacher route at the small shape and at the case's own, the prediction route through both entry points"""
    V.check_teacher(name, plan, V.NAN_SHAPE, 0, DEV, nan=True)
    V.check_teacher(name, plan, shape, 0, DEV, nan=True)
    V.check_predictions(name, plan, "encode", DEV, nan=True)
    V.check_predictions(name, plan, "forward", DEV, nan=True)
