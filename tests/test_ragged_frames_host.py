"""Ragged frame batches, the host side (no GPU): the scheduler's phase-2 grouping with ragged_frames,
the argument checks, NotImplementedError on the engines whose conv forms do not take the lengths (before any launch),
the new ctypes fields, and -- through the dispatch stand-in of tools/dispatch_trace.py -- the library's routing of
stzs_conv_args.t_lens: the two forms that honour it launch their own kernel instances, every other form or
combination (split-K, pro_part, stride, ConvTranspose, plain linear, Snake, mixed dtypes, a scalar epilogue, groups)
is refused with STZS_EINVAL and no runtime call."""
import ctypes as C
import inspect
import os
import shutil
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
TOOL = os.path.join(ROOT, "tools", "dispatch_trace.py")
OBJECTS = os.path.join(ROOT, "styletts-zs_amd", "build")


def test_phase2_groups():
    from stzs.scheduler import BucketScheduler
    frames = [24, 48, 48, 24, 40, 40, 32]
    plain = BucketScheduler(None, max_batch=4)
    assert plain.ragged_frames is False  # off by default
    pros, dec = plain.phase2_groups(frames)
    assert pros == dec == [[0, 3], [1, 2], [4, 5], [6]]  # one prosody + decoder batch per frame bucket
    rag = BucketScheduler(types.SimpleNamespace(_check_ragged_frames=lambda: None), max_batch=4, ragged_frames=True)
    pros, dec = rag.phase2_groups(frames)
    assert pros == [[0, 1, 2, 3], [4, 5, 6]]  # request order, whatever the frame counts
    assert dec == [[0, 3], [1, 2], [4, 5], [6]]
    rag.max_batch = 2
    pros, dec = rag.phase2_groups([7, 7, 7, 9, 7])
    assert pros == [[0, 1], [2, 3], [4]] and dec == [[0, 1], [2, 4], [3]]
    for g in (pros, dec):
        assert sorted(i for ch in g for i in ch) == list(range(5))


def test_keywords_and_defaults():
    from stzs.engine import StyleTTSZS
    from stzs.scheduler import BucketScheduler
    for fn in ("predict_prosody", "prosody_frames"):
        p = inspect.signature(getattr(StyleTTSZS, fn)).parameters
        assert p["ragged_frames"].default is False, fn
    assert inspect.signature(StyleTTSZS.f0n_predictor).parameters["frame_lens"].default is None
    assert inspect.signature(BucketScheduler.__init__).parameters["ragged_frames"].default is False
    assert callable(StyleTTSZS.prosody_rows)


def _engine_stub(**kw):
    """an engine object with just the attributes the ragged-frames check reads: no device, no library"""
    from stzs.engine import StyleTTSZS
    e = StyleTTSZS.__new__(StyleTTSZS)
    e.blk_splitk, e.precise, e.precise_all, e.launches = 0, False, False, 0
    for k, v in kw.items():
        setattr(e, k, v)
    return e


@pytest.mark.parametrize("kw", [dict(blk_splitk=4), dict(precise=True), dict(precise=True, precise_all=True)],
                         ids=["latency", "precise_decoder", "precise"])
def test_unsupported_engines_raise_before_any_launch(kw):
    from stzs.scheduler import BucketScheduler
    e = _engine_stub(**kw)
    for call in (lambda: e.predict_prosody(None, None, ragged_frames=True),
                 lambda: e.prosody_frames(None, None, None, None, 8, ragged_frames=True),
                 lambda: e.f0n_predictor(types.SimpleNamespace(B=1, T=8), None, frame_lens=object()),
                 lambda: BucketScheduler(e, ragged_frames=True)):
        with pytest.raises(NotImplementedError):
            call()
    assert e.launches == 0
    _engine_stub()._check_ragged_frames()  # the default engine passes
    BucketScheduler(e)  # and without the flag every engine is accepted as before


def test_abi_has_the_frame_length_fields():
    from stzs import _lib as L
    for struct, fields in ((L.ConvArgs, ("t_lens", "t_lens_mul")), (L.StatsArgs, ("lens", "lens_mul")), (L.DwupArgs, ("lens",))):
        names = [f[0] for f in struct._fields_]
        for f in fields:
            assert f in names, (struct.__name__, f)
    assert dict(L.ConvArgs._fields_)["t_lens"] is L.opt_vp and dict(L.StatsArgs._fields_)["lens"] is L.opt_vp and \
        dict(L.DwupArgs._fields_)["lens"] is L.opt_vp
    a = L.ConvArgs()
    assert not a.t_lens and a.t_lens_mul == 0  # NULL = the launch as before
    assert C.sizeof(L.ConvArgs) % 8 == 0 and C.sizeof(L.StatsArgs) % 8 == 0 and C.sizeof(L.DwupArgs) % 8 == 0


needs_objects = pytest.mark.skipif(
    shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h") or
    not os.path.exists(os.path.join(OBJECTS, "dispatch.o")),
    reason="needs g++, the HIP headers and the library's objects (styletts-zs_amd/build.py)")


@pytest.fixture(scope="module")
def tlens_calls(tmp_path_factory):
    """the sweep's t_lens calls -> [(label, return code, [launched kernel, ...], other runtime lines)]"""
    import dispatch_trace as D
    tmp = tmp_path_factory.mktemp("tlens")
    r = subprocess.run([sys.executable, TOOL, "--lib", str(tmp / "libstzs_trace.so"), "--sweep", "--out", str(tmp / "s.txt")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for kind, text, rc, lines in D.parse(tmp / "s.txt"):
        if "tlens" in text:
            out.append((text, rc, [ln.split()[1] for ln in lines if ln.startswith("L ")],
                        [ln for ln in lines if not ln.startswith("L ")]))
    return out


@needs_objects
def test_t_lens_forms_that_honour_it_launch_their_own_instances(tlens_calls):
    ok = [c for c in tlens_calls if ".bad" not in c[0]]
    assert len(ok) >= 25
    seen = set()
    for label, rc, kernels, other in ok:
        want = 2 if "pair.nosplit" in label else 1  # (a group without a shared launch: one conv after the other)
        assert rc == (2 if "pair.nosplit" in label else 0) and len(kernels) == want, (label, rc, kernels)
        for k in kernels:
            # the length-aware instances: the trailing template argument (RAG) is true
            assert ("conv_mfma" in k or "mrfv_conv" in k) and k.endswith("Lb1EEEv14stzs_conv_args"), (label, k)
            seen.add(k)
    assert sum("conv_mfma" in k for k in seen) == 4   # bf16 / fp32 x NONE / LEAKY
    assert sum("mrfv_conv" in k for k in seen) == 12  # NONE / LEAKY x residual x (64-row, 128-row, wide)


@needs_objects
def test_t_lens_everything_else_is_refused_with_no_runtime_call(tlens_calls):
    bad = [c for c in tlens_calls if ".bad" in c[0]]
    assert len(bad) >= 27
    for label, rc, kernels, other in bad:
        assert rc == -1 and not kernels and not other, (label, rc, kernels, other)  # STZS_EINVAL, nothing recorded
    labels = " | ".join(c[0] for c in bad)
    for must in ("splitk", "pro_part", "stride 2", "ups", "flat", "glds", "snake", "lane16", "narrow32", "x3frag", "rows",
                 "trio", "pair", "ks 1 shortcut", "scalar epilogue"):
        assert must in labels, must
