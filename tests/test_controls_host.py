"""Per-request controls, the host side (no GPU): row_controls' checks on an engine stub (the arrays live
on the host there), the structural errors of RowControls.set, the float64 -> fp32 pitch factor, the Request defaults,
the scheduler's grouping unchanged by the new fields, the keyword defaults of every method that takes controls, the
C layout of the grown stzs_dur_args and of stzs_row_scale_args, and the new entry points' argument checks (fake
pointers: they return before any runtime call)."""
import ctypes as C
import inspect
import os
import subprocess

import pytest
import torch

from conftest import ROOT


def _engine_stub():
    """an engine with just what row_controls reads: a device (the host), no library"""
    from stzs.engine import StyleTTSZS
    e = StyleTTSZS.__new__(StyleTTSZS)
    e.device = torch.device("cpu")
    return e


def test_row_controls_values_and_flags():
    e = _engine_stub()
    rc = e.row_controls(4, cfg_scale=[5, 1, 2.5, 0], speed=[1, 0.5, 1.7, 4.0], pitch_shift=[0, 12, -7, 3.5])
    assert rc.B == 4 and rc.cfg_form and rc.use_rate and rc.use_pitch and rc.cfg_scalar is None
    for t in (rc.cfg, rc.rate, rc.mul):
        assert t.dtype == torch.float32 and tuple(t.shape) == (4,) and t.is_contiguous()
    assert rc.cfg.tolist() == [5.0, 1.0, 2.5, 0.0]
    assert rc.rate.tolist() == torch.tensor([1, 0.5, 1.7, 4.0], dtype=torch.float32).tolist()
    want = [float(torch.tensor(2.0 ** (p / 12.0), dtype=torch.float64).float()) for p in (0.0, 12.0, -7.0, 3.5)]
    assert rc.mul.tolist() == want and want[0] == 1.0 and want[1] == 2.0
    # host tensors and scalars: a scalar rate / shift is broadcast over the rows, a scalar guidance scale stays a scalar
    rc = e.row_controls(3, cfg_scale=2.0, speed=torch.tensor([1.0, 1.25, 0.8]), pitch_shift=2)
    assert rc.cfg is None and rc.cfg_scalar == 2.0 and not rc.cfg_form
    assert rc.mul.tolist() == [float(torch.tensor(2.0 ** (2 / 12.0), dtype=torch.float64).float())] * 3
    # absent and neutral controls launch nothing
    rc = e.row_controls(2)
    assert rc.cfg is None and rc.rate is None and rc.mul is None and not (rc.cfg_form or rc.use_rate or rc.use_pitch)
    rc = e.row_controls(2, cfg_scale=[1, 1], speed=[1, 1], pitch_shift=[0, 0])
    assert not (rc.cfg_form or rc.use_rate or rc.use_pitch) and rc.cfg is not None
    assert rc.rows(2) is rc
    with pytest.raises(ValueError):
        rc.rows(3)


@pytest.mark.parametrize("kw", [
    dict(cfg_scale=[5, 1, 2]), dict(cfg_scale=[[5, 1, 2, 3]]), dict(cfg_scale=[5, 1, float("nan"), 2]),
    dict(cfg_scale=[5, 1, -0.5, 2]), dict(cfg_scale=float("inf")),
    dict(speed=[1, 1, 1]), dict(speed=[1, 0.2, 1, 1]), dict(speed=[1, 4.5, 1, 1]), dict(speed=0.0),
    dict(speed=[1, float("nan"), 1, 1]), dict(speed=[1, float("inf"), 1, 1]), dict(speed=[True, False, True, True]),
    dict(pitch_shift=[0, 25, 0, 0]), dict(pitch_shift=[0, -24.5, 0, 0]), dict(pitch_shift=[0, 0]),
    dict(pitch_shift=[0, float("nan"), 0, 0]), dict(pitch_shift="up")])
def test_row_controls_refuses(kw):
    with pytest.raises(ValueError):
        _engine_stub().row_controls(4, **kw)


def test_row_controls_range_ends_are_legal():
    rc = _engine_stub().row_controls(4, cfg_scale=[0, 0, 1, 1], speed=[0.25, 4.0, 1, 1], pitch_shift=[-24, 24, 0, 0])
    assert rc.mul.tolist() == [0.25, 4.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        _engine_stub().row_controls(0)


def test_set_rewrites_in_place_and_refuses_structural_changes():
    e = _engine_stub()
    rc = e.row_controls(2, cfg_scale=[5, 1], speed=[1, 2], pitch_shift=[0, 12])
    ptrs = [t.data_ptr() for t in (rc.cfg, rc.rate, rc.mul)]
    assert rc.set(cfg_scale=[1, 3], speed=[0.5, 1], pitch_shift=[-12, 0]) is rc
    assert [t.data_ptr() for t in (rc.cfg, rc.rate, rc.mul)] == ptrs  # the same arrays: a captured graph reads them
    assert rc.cfg.tolist() == [1.0, 3.0] and rc.rate.tolist() == [0.5, 1.0] and rc.mul.tolist() == [0.5, 1.0]
    rc.set(speed=[1, 1], pitch_shift=0)  # an active rate / shift may go back to neutral (the launches stay)
    assert rc.use_rate and rc.use_pitch and rc.rate.tolist() == [1.0, 1.0] and rc.mul.tolist() == [1.0, 1.0]
    before = (rc.cfg.clone(), rc.rate.clone(), rc.mul.clone())
    for kw in (dict(cfg_scale=[1, 1]),           # the CFG form would switch off
               dict(cfg_scale=2.0),              # per row -> a scalar launch argument
               dict(speed=[1, 5]), dict(pitch_shift=[0, 30]), dict(cfg_scale=[1, 2, 3]),
               dict(cfg_scale=[2, 2], speed=[1, 9])):  # (nothing is written when any value is refused)
        with pytest.raises(ValueError):
            rc.set(**kw)
    assert all(torch.equal(a, b) for a, b in zip(before, (rc.cfg, rc.rate, rc.mul)))
    off = e.row_controls(2, cfg_scale=[1, 1], speed=[1, 1], pitch_shift=[0, 0])
    for kw in (dict(cfg_scale=[1, 2]), dict(speed=[1, 2]), dict(pitch_shift=[0, 1])):  # neutral -> active
        with pytest.raises(ValueError):
            off.set(**kw)
    off.set(cfg_scale=[1, 1], speed=1, pitch_shift=[0, 0])
    absent = e.row_controls(2, speed=[1, 2])
    for kw in (dict(cfg_scale=[1, 2]), dict(pitch_shift=[0, 1])):  # absent -> present
        with pytest.raises(ValueError):
            absent.set(**kw)
    scalar = e.row_controls(2, cfg_scale=3.0)
    with pytest.raises(ValueError):
        scalar.set(cfg_scale=[3, 3])


def _reqs():
    from stzs.scheduler import Request
    shapes = [(10, 24000), (8, 24000), (10, 12000), (8, 24000), (10, 24000)]
    return [Request(torch.zeros(t, dtype=torch.int32), torch.zeros(n), torch.zeros(8, 64)) for t, n in shapes]


def test_request_defaults_and_grouping_unchanged():
    from stzs.scheduler import BucketScheduler
    r = _reqs()[0]
    assert r.cfg_scale is None and r.speed == 1.0 and r.pitch_shift == 0.0
    plain, mixed = _reqs(), _reqs()
    for k, q in enumerate(mixed):
        q.cfg_scale, q.speed, q.pitch_shift = [None, 1.0, 2.5, 0.0, 5.0][k], 0.8 + 0.1 * k, float(k - 2)
    frames = [24, 48, 48, 24, 40]
    eng = type("E", (), {"_check_ragged_frames": lambda self: None, "_check_ragged_decoder": lambda self: None})()
    for kw in (dict(), dict(ragged_text=True), dict(ragged_ref=True), dict(ragged_text=True, ragged_ref=True),
               dict(ragged_frames=True), dict(ragged_frames=True, ragged_decoder=True)):
        sch = BucketScheduler(eng, max_batch=2, **kw)
        assert sch.phase1_groups(mixed) == sch.phase1_groups(plain), kw
        assert sch.phase2_groups(frames) == BucketScheduler(eng, max_batch=2, **kw).phase2_groups(frames)


def test_scheduler_builds_controls_only_off_the_defaults():
    from stzs.scheduler import BucketScheduler
    made = []
    eng = type("E", (), {"row_controls": lambda self, B, **kw: made.append((B, kw)) or ("rc", B)})()
    sch = BucketScheduler(eng, max_batch=4, cfg_scale=5.0)
    sch._nctl = 0
    reqs = _reqs()
    assert sch._phase1_controls(reqs, [0, 1, 2]) is None and not made
    reqs[1].cfg_scale = 5.0  # the scheduler's own scale, spelled out: still the default
    assert sch._phase1_controls(reqs, [0, 1, 2]) is None and not made
    reqs[1].cfg_scale = 1.0
    assert sch._phase1_controls(reqs, [0, 1, 2]) == ("rc", 3)
    assert made.pop() == (3, dict(cfg_scale=[5.0, 1.0, 5.0], speed=None))
    reqs[2].speed = 1.25
    sch._phase1_controls(reqs, [2, 3])
    assert made.pop() == (2, dict(cfg_scale=5.0, speed=[1.25, 1.0]))  # a shared scale goes down as the scalar
    per = [dict(pitch=0.0), dict(pitch=0.0), dict(pitch=-3.0)]
    assert sch._phase2_controls(per, [0, 1]) == {} and not made and sch._nctl == 0
    assert sch._phase2_controls(per, [1, 2]) == dict(controls=("rc", 2)) and sch._nctl == 1
    assert made.pop() == (2, dict(pitch_shift=[0.0, -3.0]))


def test_keyword_defaults():
    from stzs.engine import RowControls, StyleTTSZS
    for fn in ("sample_style", "predict_durations", "predict_prosody", "prosody_frames", "f0n_predictor", "_front",
               "synth", "synth_stream", "duration_head"):
        p = inspect.signature(getattr(StyleTTSZS, fn)).parameters
        assert "controls" in p and p["controls"].default is None, fn
    assert inspect.signature(StyleTTSZS.synth).parameters["cfg_scale"].default == 1.0  # (stays)
    p = inspect.signature(StyleTTSZS.row_controls).parameters
    assert [p[k].default for k in ("cfg_scale", "speed", "pitch_shift")] == [None, None, None]
    p = inspect.signature(RowControls.set).parameters
    assert [p[k].default for k in ("cfg_scale", "speed", "pitch_shift")] == [None, None, None]


def test_struct_layouts_match_the_header(tmp_path):
    """gcc's sizeof / offsetof of stzs_dur_args (grown by `rate`) and stzs_row_scale_args against the ctypes mirrors"""
    from stzs import _lib as L
    structs = {"stzs_dur_args": L.DurArgs, "stzs_row_scale_args": L.RowScaleArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stzs.h"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _t in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {}
    for ln in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n"):
        if ln.strip():
            a, b, c = ln.split()
            got[(a, b)] = int(c)
    for cname, py in structs.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f, _t in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert L.DurArgs._fields_[-1] == ("rate", L.opt_vp)  # optional and trailing: NULL = the launch as before
    assert not L.DurArgs().rate


def test_new_entry_points_reject_before_launch():
    from stzs import _lib as L
    lib = L.load()
    assert "stzs_cfg_euler_rows" in L.EXPORTS and "stzs_row_scale" in L.EXPORTS
    p = C.c_void_p(0x1000)
    E, S = L.EINVAL, L.ESHAPE
    assert lib.stzs_cfg_euler_rows(p, p, 1, 1, None, 1.0, 0.5, None) == E  # scales are required
    assert lib.stzs_cfg_euler_rows(None, p, 1, 1, p, 1.0, 0.5, None) == E
    assert lib.stzs_cfg_euler_rows(p, None, 1, 1, p, 1.0, 0.5, None) == E
    assert lib.stzs_cfg_euler_rows(p, p, 0, 1, p, 1.0, 0.5, None) == S
    assert lib.stzs_cfg_euler_rows(p, p, 1, 0, p, 1.0, 0.5, None) == S
    assert lib.stzs_cfg_euler_rows(p, p, 1, 1, p, 0.0, 0.5, None) == S  # sigma must be > 0

    def args(**kw):
        a = L.RowScaleArgs()
        a.x, a.mul, a.ld, a.bs, a.B, a.T = 0x1000, 0x2000, 1, 40, 3, 37
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.stzs_row_scale(None, None) == E
    assert lib.stzs_row_scale(C.byref(args(x=None)), None) == E
    assert lib.stzs_row_scale(C.byref(args(mul=None)), None) == E
    assert lib.stzs_row_scale(C.byref(args(x=0x1002)), None) == E  # not 4-byte aligned
    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(ld=0), dict(bs=36), dict(ld=2, bs=72)):
        assert lib.stzs_row_scale(C.byref(args(**kw)), None) == S, kw
    a = L.DurArgs()
    a.logits, a.dur, a.rate = 0x1000, 0x2000, 0x3000
    a.B, a.T, a.nbins = 0, 5, 8
    assert lib.stzs_durations(C.byref(a), None) == S
    a.B, a.dur = 4, None
    assert lib.stzs_durations(C.byref(a), None) == E
