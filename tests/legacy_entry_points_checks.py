"""Checks of the older entry points of the inference C ABI against the general form each of them forwards to (include/esmi.h):

    esmi_phoneme2mel_forward_f32 / _ctl_f32 / _prec_f32       -> esmi_phoneme2mel_forward_curve_f32
    esmi_fuse_variance_adaptor_f32 / _ctl_f32                 -> esmi_fuse_variance_adaptor_curve_f32
    esmi_variance_adaptor_f32 / _ctl_f32                      -> esmi_variance_adaptor_curve_f32

The Python modules only call the general forms, so nothing else runs the older ones.  (The mel decoder pair is
precision_checks.check_entry_points.)  tests/test_legacy_entry_points.py runs the checks through the wave simulator and
on the device.  Tiny ES at prosody_control_checks.SHAPE (B = 3, T = 17, lengths (17, 9, 1)); every output buffer is filled with NaN
(its bit pattern in the int32 ones) before each call, and every comparison is `array_equal` on all of them: a NaN left anywhere fails it."""
import ctypes as C

import numpy as np
import torch

from efficientspeech_amd import _lib, networks
from tests import prosody_control_checks as P
from tests import prosody_curve_checks as Q

SHAPE = P.SHAPE
SCALES = P.SCALES                                            # three (B,) scales, every value from {0.5, 0.75, 1.25, 1.5}
PLANS = (63, 0)                                              # the one-launch enc_all16, and one kernel per op (va_tail_kernel)
assert all(v in Q.VALUES for s in SCALES.values() for v in s)


def check_scales_move_the_oracles_decisions():
    """the precondition of "ctl equals curve": on the oracle's free-running predictions (CPU, no kernel) SCALES move at least one
    live decision of each kind -- a condition of the inputs, not a measurement"""
    B, T, lens = SHAPE
    _, _, sd = P.net_of("tiny", "cpu")
    _, _, mask = P.inputs(B, T, lens, "cpu")
    o = P.free_running("tiny", SHAPE)
    raw = {k: np.ascontiguousarray(getattr(o, k)[..., 0], np.float32) for k in Q.QUANTITIES}
    scaled = Q.expected_decisions(raw, sd, mask, {k: np.asarray(v, np.float32) for k, v in SCALES.items()})
    changed = Q.changed_fraction(scaled, Q.expected_decisions(raw, sd, mask, {}), Q.live_of(mask, B, T))
    assert min(changed.values()) > 0, changed


def _nan(device, *shape, dtype=torch.float32):
    t = torch.full(shape, float("nan"), dtype=torch.float32, device=device)
    return t if dtype == torch.float32 else t.view(dtype)


def _numpy(bufs):
    return {k: v.detach().cpu().numpy() for k, v in bufs.items()}


def written(out, what):
    """no output keeps its fill"""
    for k, v in out.items():
        left = np.isnan(v) if v.dtype == np.float32 else v == np.float32("nan").view(np.int32)
        assert not left.any(), (what, k)


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


class Case:
    """tiny ES on `device` with its weights packed, the fixed phonemes, the three scales as device arrays behind both control structs"""

    def __init__(self, device):
        self.device = device
        self.net, self.cfg, _ = P.net_of("tiny", device)
        self.x, _, _ = P.inputs(*SHAPE, device)
        with torch.no_grad(), networks._on_device_of(self.net.decoder.mel_linear.weight):
            self.net(self.x)                                 # (weights packed, attributes set)
            self.lib, self.stream = networks._runtime(self.net.decoder.mel_linear.weight)
        self.ids = self.x["phoneme"].to(torch.int32).contiguous()
        self.m8 = networks._mask_u8(self.x["phoneme_mask"])
        B = SHAPE[0]
        self.scales = [torch.tensor(SCALES[k][:B], dtype=torch.float32, device=device) for k in Q.QUANTITIES]
        self.ctl, self.curves = _lib.ProsodyControl(), _lib.ProsodyCurves()          # (curves: `*_per_phoneme` stay 0)
        for struct in (self.ctl, self.curves):
            struct.pitch_scale, struct.energy_scale, struct.duration_scale = (t.data_ptr() for t in self.scales)
        self.precisions = (0, 32) if "dec_gemm=fp32-mfma" in self.lib.esmi_build_config().decode() else (0, 32, 16)

    # ------------------------------------------------------------------ the one-call forward
    def forward(self, plan, call, stages, L_out=None):
        """`call(a, stage)` -- one of the entry points on the filled esmi_forward_args -- once per stage -> every output and tap.
        L_out None (stages 1, 2 only): the batch maximum that stage 1 leaves in lmax_dev, read by the host as the reference does."""
        B, T, _ = SHAPE
        dev, lib = self.device, self.lib
        a = self.net._static_args(lib, self.stream)
        f32 = {k: _nan(dev, B, T) for k in ("duration", "pitch", "energy")}
        i32 = {k: _nan(dev, B, T, dtype=torch.int32) for k in ("pitch_idx", "energy_idx", "dur", "cum")}
        mel_len, lmax = _nan(dev, B, dtype=torch.int32), _nan(dev, 1, dtype=torch.int32)
        a.B, a.T, a.plan = B, T, plan
        a.ids, a.mask, a.dur_forced = self.ids.data_ptr(), self.m8.data_ptr(), None
        a.duration_pred, a.mel_len, a.lmax_dev = f32["duration"].data_ptr(), mel_len.data_ptr(), lmax.data_ptr()
        a.pitch_pred, a.energy_pred = f32["pitch"].data_ptr(), f32["energy"].data_ptr()
        a.pitch_idx, a.energy_idx, a.dur, a.cum = (i32[k].data_ptr() for k in ("pitch_idx", "energy_idx", "dur", "cum"))
        a.range_flag = None
        a.L_out, a.lmax_host, a.mel = L_out or 0, L_out or 0, None
        arena = torch.empty(lib.esmi_forward_arena_bytes(C.byref(a)), dtype=torch.uint8, device=dev)
        a.arena, a.arena_bytes = arena.data_ptr(), arena.numel()
        mel = None
        for stage in stages:
            if stage != 1:
                if L_out is None:
                    L_out = int(lmax.item())
                mel = _nan(dev, B, L_out, self.cfg.n_mel_channels)
                a.L_out, a.lmax_host, a.mel = L_out, L_out, mel.data_ptr()
            call(a, stage)
        return _numpy(dict(f32, **i32, mel_len=mel_len, mel=mel)), L_out

    def check_forward(self, plan):
        """every older form of the one-call forward, as one call and as stages 1 then 2, against the general form"""
        lib, st = self.lib, self.stream
        ctl, curves = C.byref(self.ctl), C.byref(self.curves)
        pairs = [("f32", lambda a, stage: lib.esmi_phoneme2mel_forward_f32(C.byref(a), stage, st), (None, 32)),
                 ("ctl_f32", lambda a, stage: lib.esmi_phoneme2mel_forward_ctl_f32(C.byref(a), ctl, stage, st), (curves, 32))]
        for prec in self.precisions:
            pairs.append((f"prec_f32 at {prec}", (lambda p: lambda a, stage: lib.esmi_phoneme2mel_forward_prec_f32(C.byref(a), None, p, stage, st))(prec),
                          (None, prec)))
        results, general = {}, {}

        def general_form(c, prec):
            """esmi_phoneme2mel_forward_curve_f32(a, c, prec, ...) as stages 1 then 2 and as one call (run once per argument pair)"""
            if (c, prec) not in general:
                call = lambda a, stage: lib.esmi_phoneme2mel_forward_curve_f32(C.byref(a), c, prec, stage, st)     # noqa: E731
                want, L = self.forward(plan, call, (1, 2))
                written(want, (c, prec))
                whole, _ = self.forward(plan, call, (0,), L)
                same(whole, want, ("the general form as one call against its stages 1, 2", prec))
                general[c, prec] = want, L
            return general[c, prec]
        with torch.no_grad(), networks._on_device_of(self.net.decoder.mel_linear.weight):
            for what, older, args in pairs:
                want, L = general_form(*args)
                assert L > 0
                same(self.forward(plan, older, (1, 2))[0], want, (what, "stages 1, 2"))
                same(self.forward(plan, older, (0,), L)[0], want, (what, "stage 0"))
                results[what] = want
        # the pairs are not one result under three names: the scales moved the decisions, precision 16 the mel
        assert not np.array_equal(results["ctl_f32"]["dur"], results["f32"]["dur"])
        assert not np.array_equal(results["ctl_f32"]["pitch_idx"], results["f32"]["pitch_idx"])
        same(results["prec_f32 at 0"], results["f32"], "precision 0")
        same(results["prec_f32 at 32"], results["f32"], "precision 32")
        if 16 in self.precisions:
            p16 = results["prec_f32 at 16"]
            assert np.array_equal(p16["mel_len"], results["f32"]["mel_len"]) and not np.array_equal(p16["mel"], results["f32"]["mel"])

    # ------------------------------------------------------------------ the two stage entry points
    def _stage_buffers(self, dim):
        B, T, _ = SHAPE
        dev = self.device
        out = dict(feat=_nan(dev, B, T, 4 * dim), preds=_nan(dev, 3, B, T), idx=_nan(dev, 2, B, T, dtype=torch.int32),
                   dur=_nan(dev, B, T, dtype=torch.int32))
        return out, [t.data_ptr() for t in (out["feat"], *out["preds"], *out["idx"], out["dur"])]

    def fuse_variance_adaptor(self, plan, entry, ctl):
        """esmi_fuse_variance_adaptor_<entry> on the encoder's feature pyramid, the decoder's phoneme-rate head included -> every output"""
        B, T, _ = SHAPE
        dev, lib, st, enc, dim = self.device, self.lib, self.stream, self.net.encoder, self.cfg.dim
        with _lib.launch_plan(plan):
            feats, bm = enc.encoder._run(self.x["phoneme"], self.x["phoneme_mask"])
        fw, _ = enc.fuse._packed(lib, st)
        (pw, _), (ew, _), (dw, _) = enc._predictors(lib, st)
        head = self.net.decoder._head(lib, st)
        out, ptrs = self._stage_buffers(dim)
        out.update(cum=_nan(dev, B, T, dtype=torch.int32), mel_len=_nan(dev, B, dtype=torch.int32), h0=_nan(dev, B, T, head[0].dx2))
        ws = torch.empty(lib.esmi_fuse_variance_adaptor_workspace_bytes(B, T, dim, len(feats)), dtype=torch.uint8, device=dev)
        fp = (C.c_void_p * len(feats))(*[f.data_ptr() for f in feats])
        ni = (C.c_int * len(feats))(*[f.shape[1] for f in feats])
        getattr(lib, "esmi_fuse_variance_adaptor_" + entry)(
            C.byref(fw), len(feats), dim, enc.fuse.kernel_size, B, T, fp, ni, C.byref(pw), C.byref(ew), C.byref(dw), bm[0].data_ptr(),
            None, None, None, *ptrs, out["cum"].data_ptr(), out["mel_len"].data_ptr(), C.byref(head[0]), out["h0"].data_ptr(), plan,
            ws.data_ptr(), ws.numel(), st, *ctl)
        return _numpy(out)

    def variance_adaptor(self, fused, entry, ctl):
        """esmi_variance_adaptor_<entry> on the fused features `fused` (B, T, dim) -> every output"""
        B, T, _ = SHAPE
        lib, st, enc, dim = self.lib, self.stream, self.net.encoder, self.cfg.dim
        (pw, _), (ew, _), (dw, _) = enc._predictors(lib, st)
        out, ptrs = self._stage_buffers(dim)
        out["feat"][..., :dim] = torch.from_numpy(fused).to(self.device)      # (channels [0, dim) are read, the others written)
        ws = torch.empty(lib.esmi_variance_adaptor_workspace_bytes(B, T, dim), dtype=torch.uint8, device=self.device)
        getattr(lib, "esmi_variance_adaptor_" + entry)(C.byref(pw), C.byref(ew), C.byref(dw), dim, B, T, self.m8.data_ptr(), None, None, None,
                                                       *ptrs, ws.data_ptr(), ws.numel(), st, *ctl)
        return _numpy(out)

    def check_stages(self, plan):
        """esmi_fuse_variance_adaptor_{f32, ctl_f32} and esmi_variance_adaptor_{f32, ctl_f32} against their _curve_f32 forms"""
        ctl, curves, dim = C.byref(self.ctl), C.byref(self.curves), self.cfg.dim
        with torch.no_grad(), networks._on_device_of(self.net.decoder.mel_linear.weight):
            plain = self.fuse_variance_adaptor(plan, "curve_f32", (None,))
            scaled = self.fuse_variance_adaptor(plan, "curve_f32", (curves,))
            written(plain, "esmi_fuse_variance_adaptor_curve_f32")
            same(self.fuse_variance_adaptor(plan, "f32", ()), plain, "esmi_fuse_variance_adaptor_f32")
            same(self.fuse_variance_adaptor(plan, "ctl_f32", (ctl,)), scaled, "esmi_fuse_variance_adaptor_ctl_f32")
            assert not np.array_equal(scaled["dur"], plain["dur"]) and not np.array_equal(scaled["idx"], plain["idx"])
            fused = plain["feat"][..., :dim]
            va_plain = self.variance_adaptor(fused, "curve_f32", (None,))
            va_scaled = self.variance_adaptor(fused, "curve_f32", (curves,))
            written(va_plain, "esmi_variance_adaptor_curve_f32")
            same(self.variance_adaptor(fused, "f32", ()), va_plain, "esmi_variance_adaptor_f32")
            same(self.variance_adaptor(fused, "ctl_f32", (ctl,)), va_scaled, "esmi_variance_adaptor_ctl_f32")
            assert not np.array_equal(va_scaled["dur"], va_plain["dur"]) and not np.array_equal(va_scaled["idx"], va_plain["idx"])
