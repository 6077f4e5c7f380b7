"""Checks of the variance adaptor's discrete decisions at exact ties: values ON a bucket edge and one fp32 step beside it, duration
products ON a .5.  tests/test_va_ties.py runs them twice: through the wave simulator (host tensors, inside `tests.simlib.use_sim()`)
and on the device.

The expectation always comes from the reference's own operators on the CPU -- torch.bucketize(v, bins) (right=False), torch.round,
masked_fill, clamp(min=0), .int(), F.embedding -- and every decision is compared bit for bit: nothing here has a tolerance except the
one mel comparison per config (helpers.MEL_TOL) and the embedding gradient (2e-5, test_train_ops._close).

Two routes put an exact value in front of a kernel's comparison:
  * teacher: `_encode(x, train=True)` bucketizes x["pitch"] / x["energy"] as given;
  * prediction: with a predictor's output `linear.weight` zeroed its raw prediction is `linear.bias` bit for bit (sums of exact zeros
    plus the bias), and a (B,) control tensor -- tensors are not validated on the host -- puts `bias * s[b]` where it is wanted.

Every case also computes its expectation under the WRONG rules (side="right"; floor(x + .5)) and asserts that they differ from the right
one on enough rows: inputs on which a wrong kernel would still pass are refused.  The third wrong rule one might think of, the clamp
before the rounding instead of after it, is not observable on any input: torch.round is monotone and round(0) == 0, so
round(max(x, 0)) == max(round(x), 0) for every x; `wrong_rules_duration` asserts that identity instead.  What a stray clamp WOULD
change is the B == 1 call without a mask (no clamp there, as in the reference): `check_single_utterance`.

NaN (check_nan_*): `e < NaN` is false for every edge, so a NaN value gets bucket 0 in every kernel and in the C oracle, inside the
table; torch.bucketize gives dim - 1.  Pinned as the project's rule (va_decide.h).  NaN DURATIONS without a mask are
left out: (int)NaN is not defined."""
import numpy as np
import torch
import torch.nn.functional as F

from efficientspeech_amd import CONFIGS, _lib, build_phoneme2mel, load_numpy_state_dict, networks
from efficientspeech_amd.synth import synth_phonemes, synth_state_dict
from oracle import oracle
from tests import helpers as H

SEED = 1234
INF = float("inf")
# B, T, lengths: the smallest shapes whose live rows hold all of V; the last utterance a few rows short
TEACHER_SHAPES = {"tiny": (2, 60, (60, 55)), "small": (2, 110, (110, 105)), "base": (4, 100, (100, 100, 100, 95))}
HALO_SHAPES = {"tiny": (2, 130, (130, 125)), "small": (2, 260, (260, 255))}      # enc_fuse_va's halo workgroups
NAN_SHAPE = (2, 20, (20, 17))
ROLLS = (0, 13)                                   # 13 is coprime to the 16- and 32-row tiles: every edge on two rows / lanes of a tile
PRED_T, PRED_LENS, PRED_CHUNK = 5, (5, 3, 1), 32
PITCH_BIAS, ENERGY_BIAS, DUR_BIAS = 1.0, 1.0, 0.5

_nets = {}
_cases = {}


def clear():
    _nets.clear(), _cases.clear()


# ------------------------------------------------------------------------------------------------------------------ inputs
def _next(v, toward):
    return torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(toward, dtype=torch.float32))


def values(bins):
    """V(bins): every edge with its two fp32 neighbours, e_0 - 1, e_last + 1, +-inf, +-0, +-3e38, +-the smallest denormal"""
    e = torch.as_tensor(bins, dtype=torch.float32).detach().cpu()
    lo, hi = torch.nextafter(e, torch.full_like(e, -INF)), torch.nextafter(e, torch.full_like(e, INF))
    extra = torch.tensor([float(e[0]) - 1.0, float(e[-1]) + 1.0, INF, -INF, 0.0, -0.0, 3e38, -3e38, 1.4e-45, -1.4e-45], dtype=torch.float32)
    v = torch.cat([torch.stack([lo, e, hi], 1).reshape(-1), extra])
    assert v.numel() == 3 * e.numel() + 10 and (lo < e).all() and (e < hi).all() and extra[8] > 0 and extra[9] < 0
    assert len(set(v.view(torch.int32).tolist())) == v.numel()            # (103 / 199 / 391 different bit patterns)
    return v


def duration_scales():
    """0 .. 15 (products 0, .5, 1, ... 7.5 of the bias .5), both fp32 neighbours of 5 and of 3 (both sides of 2.5 and 1.5), and -3
    (-1.5 rounds to -2 and is clamped to 0 under the mask)"""
    return torch.cat([torch.arange(16, dtype=torch.float32),
                      torch.stack([_next(5.0, -INF), _next(5.0, INF), _next(3.0, -INF), _next(3.0, INF)]), torch.tensor([-3.0])])


def state_dict_of(name, kind, dur_bias=DUR_BIAS):
    """kind "synth": synth_state_dict; "zero": the three predictors' output Linear zeroed, biases 1 / 1 / dur_bias"""
    sd = synth_state_dict(CONFIGS[name], SEED)
    if kind == "zero":
        for which, b in (("pitch", PITCH_BIAS), ("energy", ENERGY_BIAS), ("duration", dur_bias)):
            sd[f"encoder.{which}_decoder.linear.weight"][:] = 0.0
            sd[f"encoder.{which}_decoder.linear.bias"][:] = np.float32(b)
    return sd


def net_of(name, device, kind="synth"):
    if (name, device, kind) not in _nets:
        sd = state_dict_of(name, kind)
        net = build_phoneme2mel(CONFIGS[name])
        load_numpy_state_dict(net, sd)
        _nets[name, device, kind] = (net.to(device), CONFIGS[name], sd)
    return _nets[name, device, kind]


def tables(sd):
    """(pitch bins, energy bins, pitch table, energy table) as host tensors"""
    t = lambda k: torch.from_numpy(np.asarray(sd[k], np.float32))       # noqa: E731
    return (t("encoder.pitch_decoder.pitch_bins"), t("encoder.energy_decoder.energy_bins"),
            t("encoder.pitch_decoder.pitch_embedding.weight"), t("encoder.energy_decoder.energy_embedding.weight"))


def bucketize(v, bins, right=False):
    """torch.bucketize, and the project's NaN rule on top: no edge is below a NaN -> bucket 0 (torch: dim - 1)"""
    idx = torch.bucketize(v, bins, right=right)
    return torch.where(torch.isnan(v), torch.zeros_like(idx), idx).to(torch.int32)


def _bits(t):
    return set(t.contiguous().view(torch.int32).reshape(-1).tolist())


def wrong_rules_bucket(v, bins, live, dim):
    """6. side="right" must differ from side="left" on at least dim - 1 live rows, else the inputs could not fail"""
    n = int(((bucketize(v, bins) != bucketize(v, bins, right=True)) & live).sum())
    assert n >= dim - 1, (n, dim)


def wrong_rules_duration(prod):
    """6. (B,) products: floor(x + .5) must round at least 4 utterances differently; the clamp before the rounding cannot differ"""
    away = torch.floor(prod + 0.5)
    n = int((away != torch.round(prod)).sum())
    assert n >= 4, n
    assert torch.equal(torch.round(prod.clamp(min=0)), torch.round(prod).clamp(min=0))
    return n


# ------------------------------------------------------------------------------------------------------------------ 1. teacher route
def teacher_case(name, shape, roll, device, nan=False):
    """-> (x for `_encode(x, train=True)`, expected pitch_idx, energy_idx (B,T) int32, live (B,T) bool).  V(pitch_bins) tiled over the
    B*T rows rolled by `roll`, V(energy_bins) reversed the same way (the two indices differ per row), durations all ones.
    nan: a NaN on every 7th pitch row and every 5th energy row."""
    B, T, lens = shape
    _, cfg, sd = net_of(name, device)
    pb, eb, _, _ = tables(sd)
    ids, mask = synth_phonemes(B, T, SEED, list(lens))
    live = torch.from_numpy(~mask)
    vp, ve = values(pb), values(eb).flip(0)
    at = (torch.arange(B * T) + roll) % vp.numel()
    pitch, energy = vp[at].reshape(B, T).clone(), ve[at].reshape(B, T).clone()
    if nan:
        pitch.view(-1)[::7] = float("nan")
        energy.view(-1)[::5] = float("nan")
        assert int((torch.isnan(pitch) & live).sum()) >= 4 and int((torch.isnan(energy) & live).sum()) >= 4
        assert (torch.bucketize(pitch[torch.isnan(pitch)], pb) == cfg.dim - 1).all()        # (torch's answer, which is NOT the project's)
    else:
        assert _bits(vp) <= _bits(pitch[live]) and _bits(ve) <= _bits(energy[live])          # every value of V sits on a live row
        wrong_rules_bucket(pitch, pb, live, cfg.dim)
        wrong_rules_bucket(energy, eb, live, cfg.dim)
    x = {"phoneme": torch.from_numpy(ids).to(device), "phoneme_mask": torch.from_numpy(mask).to(device),
         "pitch": pitch.to(device), "energy": energy.to(device), "duration": torch.ones((B, T), dtype=torch.int32, device=device)}
    return x, bucketize(pitch, pb), bucketize(energy, eb), live


def check_teacher(name, plan, shape, roll, device, nan=False):
    """1. (5. with nan) `_encode(x, train=True)`: both indices on live rows, both embedding slices of `feat` bit for bit, zeros on padding"""
    net, cfg, sd = net_of(name, device)
    _, _, pt, et = tables(sd)
    x, pi, ei, live = teacher_case(name, shape, roll, device, nan)
    with torch.no_grad(), _lib.launch_plan(plan), networks._on_device_of(net.decoder.mel_linear.weight):
        enc = net.encoder._encode(x, train=True)
    got_p, got_e, feat = enc["pitch_idx"].cpu(), enc["energy_idx"].cpu(), enc["feat"].cpu()
    dim = cfg.dim
    for what, got, exp, table, lo in (("pitch", got_p, pi, pt, dim), ("energy", got_e, ei, et, 2 * dim)):
        bad = (got != exp) & live
        assert not bad.any(), (name, plan, shape, roll, what, [(r, int(got[tuple(r)]), int(exp[tuple(r)])) for r in bad.nonzero().tolist()[:8]])
        assert int(got[live].min()) >= 0 and int(got[live].max()) <= dim - 1
        sl = feat[..., lo:lo + dim]
        assert torch.equal(sl[live], table[exp.long()][live]), (name, plan, what, "embedding rows")
        assert not sl[~live].any(), (name, plan, what, "padded rows")
    if nan:
        assert (got_p[torch.isnan(x["pitch"].cpu()) & live] == 0).all() and (got_e[torch.isnan(x["energy"].cpu()) & live] == 0).all()
    assert torch.equal(enc["dur"].cpu(), live.to(torch.int32))           # (teacher durations: ones, zero under the mask)


# ------------------------------------------------------------------------------------------------------------------ 2. prediction route
def prediction_case(name, nan=False):
    """The utterances of a config's prediction run, in calls of at most 32 -> list of chunks, each a dict of host tensors: ids, mask,
    the three (B,) controls and the expected products / decisions.  Utterance u carries V(pitch_bins)[u], V(energy_bins) reversed [u],
    duration scale u mod 21, length (5, 3, 1)[u mod 3].  nan: one chunk, a NaN pitch control on every 3rd and a NaN energy control on
    every 4th utterance."""
    if (name, nan) in _cases:
        return _cases[name, nan]
    cfg = CONFIGS[name]
    pb, eb, _, _ = tables(state_dict_of(name, "zero"))
    sp, se, ds = values(pb), values(eb).flip(0), duration_scales()
    if nan:
        sp, se = sp[:PRED_CHUNK].clone(), se[:PRED_CHUNK].clone()
        sp[::3], se[::4] = float("nan"), float("nan")
    n = sp.numel()
    sd_ = ds[torch.arange(n) % ds.numel()]
    lens = torch.tensor(PRED_LENS)[torch.arange(n) % 3]
    chunks, n_side, n_round = [], [0, 0], 0
    for c0 in range(0, n, PRED_CHUNK):
        u = slice(c0, min(c0 + PRED_CHUNK, n))
        B, T = u.stop - u.start, PRED_T
        assert B > 1
        ids, mask = synth_phonemes(B, T, SEED + c0, lens[u].tolist())
        m = torch.from_numpy(mask)
        one = torch.ones((B, T), dtype=torch.float32)
        vp = one * (torch.tensor(PITCH_BIAS, dtype=torch.float32) * sp[u])[:, None]          # fp32(bias) * s[b]: 1.0 * e == e
        ve = one * (torch.tensor(ENERGY_BIAS, dtype=torch.float32) * se[u])[:, None]
        prod = torch.tensor(DUR_BIAS, dtype=torch.float32) * sd_[u]
        assert _bits(vp[:, 0]) == _bits(sp[u]) and _bits(ve[:, 0]) == _bits(se[u])
        dur = (one * torch.round(prod)[:, None]).masked_fill(m, 0).clamp(min=0).int()
        cum = torch.cumsum(dur, 1).int()
        chunks.append(dict(ids=ids, mask=mask, live=~m, vp=vp, ve=ve, prod=prod, pi=bucketize(vp, pb), ei=bucketize(ve, eb), dur=dur, cum=cum,
                           mel_len=cum[:, -1].clone(), ctl={"pitch_control": sp[u].clone(), "energy_control": se[u].clone(),
                                                            "duration_control": sd_[u].clone()}))
        for q, (v, b) in enumerate(((vp, pb), (ve, eb))):
            n_side[q] += int(((bucketize(v, b) != bucketize(v, b, right=True)) & ~m).sum())
        n_round += int((torch.floor(prod + 0.5) != torch.round(prod)).sum())
    if not nan:                                                          # 6. over the case (every full call alone has its 4 as well)
        assert min(n_side) >= cfg.dim - 1, n_side
        assert wrong_rules_duration(torch.cat([ch["prod"] for ch in chunks])) == n_round
        for ch in chunks[:-1]:
            wrong_rules_duration(ch["prod"])
        assert {0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, -1.5} <= set(chunks[0]["prod"].tolist())
    _cases[name, nan] = chunks
    return chunks


def run(net, x, entry, plan, decode=True):
    """One inference call -> dict of host tensors: the raw predictions pitch / energy / duration (B,T), the decisions pitch_idx,
    energy_idx, dur, cum (B,T), mel_len (B) and, for entry "forward" (the one-call forward with its taps), the mel.  decode=False: the
    one-call forward's encoder side alone (stage 1: the call the whole forward begins with when no output length is given), no mel."""
    c = lambda t: t.detach().cpu()      # noqa: E731
    with torch.no_grad(), _lib.launch_plan(plan), networks._on_device_of(net.decoder.mel_linear.weight):
        if entry == "forward":
            st = net._launch(x, stage=0 if decode else 1, taps=True)
            out = {k: c(v) for k, v in st.taps.items()}
            out.update(duration=c(st.duration)[..., 0], mel_len=c(st.mel_len), mel=c(st.mel) if decode else None)
        else:
            enc = net.encoder._encode(x)
            out = {k: c(enc[k]) for k in ("pitch_idx", "energy_idx", "dur", "cum", "mel_len")}
            out.update({k: c(enc[k])[..., 0] for k in ("pitch", "energy", "duration")})
    return out


def _x_of(ch, device):
    x = {"phoneme": torch.from_numpy(ch["ids"]).to(device), "phoneme_mask": torch.from_numpy(ch["mask"]).to(device)}
    x.update({k: v.to(device) for k, v in ch["ctl"].items()})
    return x


def _check_decisions(got, ch, where):
    live = ch["live"]
    for k, b in (("pitch", PITCH_BIAS), ("energy", ENERGY_BIAS), ("duration", DUR_BIAS)):     # the precondition: prediction == bias, bit for bit
        assert _bits(got[k][live]) == _bits(torch.tensor([b], dtype=torch.float32)), (where, k, "the output Linear did not give its bias")
    for k, e in (("pitch_idx", ch["pi"]), ("energy_idx", ch["ei"])):
        bad = (got[k] != e) & live
        assert not bad.any(), (where, k, [(r, int(got[k][tuple(r)]), int(e[tuple(r)])) for r in bad.nonzero().tolist()[:8]])
    for k in ("dur", "cum", "mel_len"):
        assert torch.equal(got[k], ch[k]), (where, k, got[k].tolist(), ch[k].tolist())


def check_predictions(name, plan, entry, device, chunks=None, mel=False, nan=False, decode=None, plain=True):
    """2. (5. with nan) the zero-Linear checkpoint under (B,) controls, per call of `prediction_case`: precondition, indices, durations,
    scan and mel_len bit for bit.  entry "forward" also runs the plain `net(x)` (same mel_len, duration and mel as the tapped call);
    mel: the first decoded call's mel against the oracle teacher-forced on the same products and expected durations, at helpers.MEL_TOL.
    decode: the calls whose decoder runs too (default: all).  The decisions are the encoder side's, so the simulated twins run the
    decoder -- frame-rate work, most of a simulated forward's cost -- on the last, shortest call only; the device runs it on every call.
    plain=False (simulated base ES, 6 s a decoded call): without the plain call."""
    net, cfg, sd = net_of(name, device, "zero")
    case = prediction_case(name, nan)
    decode = None if decode is None else [c % len(case) for c in decode]
    for c in (range(len(case)) if chunks is None else chunks):
        ch = case[c]
        x = _x_of(ch, device)
        full = entry == "forward" and (decode is None or c in decode)
        got = run(net, x, entry, plan, decode=full)
        _check_decisions(got, ch, (name, plan, entry, c))
        if nan:
            assert (got["pitch_idx"][torch.isnan(ch["vp"]) & ch["live"]] == 0).all() and (got["energy_idx"][torch.isnan(ch["ve"]) & ch["live"]] == 0).all()
        if full:
            if plain:
                with torch.no_grad(), _lib.launch_plan(plan):
                    m, ml, dp = net(x)
                assert torch.equal(ml.cpu(), got["mel_len"]) and torch.equal(dp.cpu()[..., 0], got["duration"]) and torch.equal(m.cpu(), got["mel"])
            for b in range(len(got["mel_len"])):
                assert not got["mel"][b, int(got["mel_len"][b]):].any(), b
            if mel and c == (0 if decode is None else decode[0]):
                o = oracle.phoneme2mel(cfg, oracle.Weights(sd), ch["ids"], ch["mask"], pitch=ch["vp"].numpy(), energy=ch["ve"].numpy(),
                                       duration=ch["dur"].numpy())
                assert np.array_equal(o.pitch_idx, ch["pi"].numpy()) and np.array_equal(o.energy_idx, ch["ei"].numpy())
                assert np.array_equal(o.mel_len, ch["mel_len"].numpy()) and tuple(got["mel"].shape) == o.mel.shape
                err = float(np.abs(got["mel"].numpy() - o.mel).max())
                print(f"{name} plan {plan}: mel L-inf vs the teacher-forced oracle {err:.2e}")
                assert err < H.MEL_TOL, err


def check_single_utterance(name, plan, entry, device):
    """2. B == 1 takes no mask: scale 3 gives 2 frames per phoneme; scale -3 stores -2 (no clamp without a mask, as in the reference),
    a scan of zeros, mel_len 0 and an empty mel."""
    net, cfg, sd = net_of(name, device, "zero")
    pb, eb, _, _ = tables(sd)
    T = PRED_T
    ids, _ = synth_phonemes(1, T, SEED)
    edge_p, edge_e = pb[cfg.dim // 2].reshape(1), eb[-1].reshape(1)
    for scale, d, total in ((3.0, 2, 2 * T), (-3.0, -2, 0)):
        x = {"phoneme": torch.from_numpy(ids).to(device), "pitch_control": edge_p.to(device), "energy_control": edge_e.to(device),
             "duration_control": torch.tensor([scale], device=device)}
        got = run(net, x, entry, plan)
        where = (name, plan, entry, scale)
        assert _bits(got["duration"]) == _bits(torch.tensor([DUR_BIAS])) and _bits(got["pitch"]) == _bits(torch.tensor([PITCH_BIAS])), where
        assert int(torch.round(torch.tensor(DUR_BIAS) * scale)) == d
        assert (got["dur"] == d).all(), (where, got["dur"].tolist())
        assert torch.equal(got["cum"], torch.cumsum(torch.full((1, T), max(d, 0)), 1).int()), (where, got["cum"].tolist())
        assert got["mel_len"].tolist() == [total], (where, got["mel_len"].tolist())
        assert (got["pitch_idx"] == int(torch.bucketize(edge_p, pb))).all() and (got["energy_idx"] == int(torch.bucketize(edge_e, eb))).all(), where
        if entry == "forward":
            assert tuple(got["mel"].shape) == (1, total, 80), (where, tuple(got["mel"].shape))
            with torch.no_grad(), _lib.launch_plan(plan):
                m, ml, _ = net(x)
            assert torch.equal(m.cpu(), got["mel"]) and ml.tolist() == [total], where


# ------------------------------------------------------------------------------------------------------------------ 3. bucket_embed_kernel
def embed_targets(bins, nan=False):
    """V as the target at shapes (|V|,), (1, 1) (the last edge) and (2, ceil(|V| / 2)) padded with edges"""
    v = values(bins)
    if nan:
        v = v.clone()
        v[::6] = float("nan")
    two = torch.cat([v, bins[:(-v.numel()) % 2]]).reshape(2, -1)
    return [v, bins[-1].reshape(1, 1).clone(), two]


def check_bucket_embed(name, device, nan=False):
    """3. (5. with nan) AcousticDecoder.get_embedding(pred, target, mask) for pitch and energy, target and prediction spelling"""
    net, cfg, sd = net_of(name, device)
    pb, eb, pt, et = tables(sd)
    for dec, bins, table in ((net.encoder.pitch_decoder, pb, pt), (net.encoder.energy_decoder, eb, et)):
        for t in embed_targets(bins, nan):
            if not nan and t.numel() > 1:
                wrong_rules_bucket(t, bins, torch.ones_like(t, dtype=torch.bool), cfg.dim)
            ref = F.embedding(bucketize(t, bins).long(), table)
            with torch.no_grad():
                got = dec.get_embedding(None, t.to(device), None)
                got_p = dec.get_embedding(t[..., None].to(device), None, None)
            assert got.shape == ref.shape and torch.equal(got.cpu(), ref), (name, tuple(t.shape))
            assert torch.equal(got_p.cpu()[..., 0, :], ref), (name, tuple(t.shape), "prediction spelling")


def check_train_bucket_embed(name, device, nan=False):
    """3. (5. with nan) train._bucket_embedding (the training step bucketizes its targets with it): the rows, and the gradient with
    respect to the table for a random dy -- a wrong bucket moves a whole gradient row"""
    from efficientspeech_amd import train
    from tests.test_train_ops import _close
    net, cfg, sd = net_of(name, device)
    pb, eb, pt, et = tables(sd)
    g = torch.Generator().manual_seed(SEED)
    for dec, emb, bins, table in ((net.encoder.pitch_decoder, net.encoder.pitch_decoder.pitch_embedding, pb, pt),
                                  (net.encoder.energy_decoder, net.encoder.energy_decoder.energy_embedding, eb, et)):
        for t in embed_targets(bins, nan):
            idx = bucketize(t, bins).long()
            tref = table.clone().requires_grad_()
            ref = F.embedding(idx, tref)
            got = train._bucket_embedding(dec, t.to(device))
            assert got.shape == ref.shape and torch.equal(got.detach().cpu(), ref.detach()), (name, tuple(t.shape))
            dy = torch.randn(ref.shape, generator=g)
            gg = torch.autograd.grad(got, emb.weight, dy.to(device))[0]
            _close(gg.cpu(), torch.autograd.grad(ref, tref, dy)[0], 2e-5, (name, tuple(t.shape), "embedding grad"))


# ------------------------------------------------------------------------------------------------------------------ 4. the oracle
def check_oracle_teacher(name, nan=False):
    """4. (5.) oracle.phoneme_encoder teacher-forced with V gives torch.bucketize's indices (NaN: bucket 0)"""
    _, cfg, sd = net_of(name, "cpu")
    x, pi, ei, live = teacher_case(name, NAN_SHAPE if nan else TEACHER_SHAPES[name], 0, "cpu", nan)
    o = oracle.phoneme_encoder(cfg, oracle.Weights(sd), x["phoneme"].numpy(), x["phoneme_mask"].numpy(), pitch=x["pitch"].numpy(),
                               energy=x["energy"].numpy(), duration=x["duration"].numpy())
    assert torch.equal(torch.from_numpy(o.pitch_idx)[live], pi[live]) and torch.equal(torch.from_numpy(o.energy_idx)[live], ei[live])


def check_oracle_rounding():
    """4. the oracle's eval run on the zero-Linear checkpoint, duration bias .5 / 1.5 / 2.5 / 3.5 -> 0, 2, 2, 4 on live rows"""
    cfg = CONFIGS["tiny"]
    ids, mask = synth_phonemes(2, 3, SEED, [3, 2])
    for bias, d in ((0.5, 0), (1.5, 2), (2.5, 2), (3.5, 4)):
        assert int(torch.round(torch.tensor(bias))) == d
        o = oracle.phoneme2mel(cfg, oracle.Weights(state_dict_of("tiny", "zero", bias)), ids, mask)
        assert _bits(torch.from_numpy(o.duration[..., 0][~mask])) == _bits(torch.tensor([bias])), bias
        assert np.array_equal(o.dur, np.where(mask, 0, d)), (bias, o.dur.tolist())
        assert o.mel_len.tolist() == [3 * d, 2 * d]
