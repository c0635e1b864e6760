"""The ragged decoder, the host side (no GPU): the new and renamed ctypes fields against the header's
layout, _check_ragged_decoder's refusals before any launch (the latency engine, the precise engines, a spec whose
generator is on the generic conv path), the scheduler's argument check and phase-2 grouping with ragged_decoder, and
-- through the dispatch stand-in of tools/dispatch_trace.py -- the library's routing of stzs_conv_args.t_lens with
t_lens_rows = 1: the three forms that honour it launch kernel instances of their own (the RAG template argument
true), every other form or combination is refused with STZS_EINVAL and no runtime call."""
import ctypes as C
import inspect
import os
import shutil
import subprocess
import sys
import tempfile
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
TOOL = os.path.join(ROOT, "tools", "dispatch_trace.py")
OBJECTS = os.path.join(ROOT, "styletts-zs_amd", "build")


def test_abi_fields_and_layout():
    """t_lens_rows sits where pad_tl sat (stzs_conv_args did not grow); the trailing optional `lens` of the source and
    iSTFT structs and stzs_frame_rows_args match the header; NULL / 0 is the launch as before"""
    from stzs import _lib as L
    names = [f[0] for f in L.ConvArgs._fields_]
    assert names[-3:] == ["t_lens", "t_lens_mul", "t_lens_rows"] and "pad_tl" not in names
    assert L.ConvArgs.t_lens_rows.offset == L.ConvArgs.t_lens_mul.offset + 4 == C.sizeof(L.ConvArgs) - 4
    for S in (L.SourceArgs, L.IstftArgs):
        assert S._fields_[-1][0] == "lens" and S._fields_[-1][1] is L.opt_vp and C.sizeof(S) % 8 == 0
    a, s, i = L.ConvArgs(), L.SourceArgs(), L.IstftArgs()
    assert a.t_lens_rows == 0 and not a.t_lens and not s.lens and not i.lens
    assert "stzs_frame_rows" in L.EXPORTS
    structs = {"stzs_conv_args": L.ConvArgs, "stzs_source_args": L.SourceArgs, "stzs_istft_args": L.IstftArgs,
               "stzs_frame_rows_args": L.FrameRowsArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stzs.h"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _t in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in
               subprocess.run([exe], capture_output=True, text=True).stdout.splitlines() if ln.strip()}
    for cname, py in structs.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f, _t in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)


def test_keywords_and_defaults():
    from stzs.engine import StyleTTSZS
    from stzs.scheduler import BucketScheduler
    sig = lambda fn: inspect.signature(getattr(StyleTTSZS, fn)).parameters
    assert sig("decode")["frame_lens"].default is None and sig("decoder_pre")["frame_lens"].default is None
    assert sig("synth")["ragged_frames"].default is False
    for fn, kw in (("sine_gen", "lens"), ("upsample", "rows"), ("mrf", "rows"), ("conv_post", "rows"), ("istft", "lens"),
                   ("generator", "rows")):
        assert sig(fn)[kw].default is None, fn
    assert sig("conv")["t_lens_rows"].default == 0
    assert inspect.signature(BucketScheduler.__init__).parameters["ragged_decoder"].default is False


def _engine_stub(**kw):
    """an engine object with just the attributes the ragged-decoder check reads: no device, no library"""
    from stzs.engine import StyleTTSZS
    e = StyleTTSZS.__new__(StyleTTSZS)
    e.blk_splitk, e.precise, e.precise_all, e.launches, e.dec_dt = 0, False, False, 0, torch.bfloat16
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _packed(spec):
    from stzs.params import init_params
    from stzs.weights import PackedModel
    return PackedModel(spec, init_params(spec, seed=0), torch.device("cpu"), fill=False)


@pytest.mark.parametrize("kw", [dict(blk_splitk=4), dict(precise=True, precise_all=True), dict(dec_dt=torch.float32),
                                dict(W="tiny")], ids=["latency", "precise", "fp32_decoder", "spec_tiny"])
def test_unsupported_engines_and_specs_raise_before_any_launch(kw, tiny):
    from stzs.scheduler import BucketScheduler
    if kw.get("W") == "tiny":
        kw = dict(W=_packed(tiny))  # (SPEC_TINY: gen_ch 32 / 16, the generic conv_mfma path)
    e = _engine_stub(**kw)
    for call in (lambda: e._check_ragged_decoder(),
                 lambda: e.decode(dict(T40=8), None, None, frame_lens=object()),
                 lambda: e.synth(None, None, ragged_frames=True),
                 lambda: BucketScheduler(e, ragged_frames=True, ragged_decoder=True)):
        with pytest.raises(NotImplementedError):
            call()
    assert e.launches == 0


def test_the_smallest_qualifying_spec_passes(tiny):
    from stzs.spec import SPEC_V0
    S = tiny.replace(dec_out=128, gen_ch=(256, 128))
    _engine_stub(W=_packed(S))._check_ragged_decoder()
    assert SPEC_V0.gen_ch[-1] == 128 and all(c in (128, 256) for c in SPEC_V0.gen_ch)  # (SPEC_V0: the same forms)


def test_scheduler_flag_and_grouping():
    from stzs.scheduler import BucketScheduler
    ok = types.SimpleNamespace(_check_ragged_frames=lambda: None, _check_ragged_decoder=lambda: None)
    with pytest.raises(ValueError):
        BucketScheduler(ok, ragged_decoder=True)  # requires ragged_frames
    assert BucketScheduler(ok).ragged_decoder is False
    sch = BucketScheduler(ok, max_batch=4, ragged_frames=True, ragged_decoder=True)
    frames = [24, 48, 48, 24, 40, 40, 32]
    pros, dec = sch.phase2_groups(frames)
    assert pros == dec == [[0, 3, 6, 4], [5, 1, 2]]  # sorted by frame count (stable), chunks of max_batch
    assert [[frames[i] for i in ch] for ch in dec] == [[24, 24, 32, 40], [40, 48, 48]]
    sch.max_batch = 2
    pros, dec = sch.phase2_groups([7, 9, 7, 1, 7])
    assert pros == dec == [[3, 0], [2, 4], [1]]
    # without the flag the §2d grouping is untouched
    assert BucketScheduler(ok, max_batch=4, ragged_frames=True).phase2_groups(frames)[1] == [[0, 3], [1, 2], [4, 5], [6]]


needs_objects = pytest.mark.skipif(
    shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h") or
    not os.path.exists(os.path.join(OBJECTS, "dispatch.o")),
    reason="needs g++, the HIP headers and the library's objects (styletts-zs_amd/build.py)")


@pytest.fixture(scope="module")
def trows_calls(tmp_path_factory):
    """the sweep's t_lens_rows = 1 calls -> [(label, return code, [launched kernel, ...], other runtime lines)]"""
    import dispatch_trace as D
    tmp = tmp_path_factory.mktemp("trows")
    r = subprocess.run([sys.executable, TOOL, "--lib", str(tmp / "libstzs_trace.so"), "--sweep", "--out", str(tmp / "s.txt")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for kind, text, rc, lines in D.parse(tmp / "s.txt"):
        if "trows" in text:
            assert "tlens" not in text
            out.append((text, rc, [ln.split()[1] for ln in lines if ln.startswith("L ")],
                        [ln for ln in lines if not ln.startswith("L ")]))
    return out


@needs_objects
def test_row_count_forms_launch_their_own_instances(trows_calls):
    ok = [c for c in trows_calls if ".bad" not in c[0]]
    assert len(ok) >= 100
    seen = set()
    for label, rc, kernels, other in ok:
        want = 3 if "trio" in label else 1  # (a group with lengths: one conv after the other, never the trio launch)
        assert rc == (3 if "trio" in label else 0) and len(kernels) == want, (label, rc, kernels)
        for k in kernels:
            # the length-aware instances: the trailing template argument (RAG) is true
            assert any(n in k for n in ("mrfv_conv", "ups_conv", "narrow_conv")) and "mrfv_trio" not in k, (label, k)
            assert k.endswith("Lb1EEEv14stzs_conv_args") or k.endswith("Lb1EEEv14stzs_conv_argsi"), (label, k)
            seen.add(k)
    # Snake: (plain, residual, residual + alpha, residual + accumulate + alpha) x k 3 / 7 / 11 x (single-chunk, narrow,
    # wide), all at 128-row tiles; ConvTranspose: 1..4 chunks x (plain, residual, fused noise); the narrow conv
    assert sum("mrfv_conv" in k for k in seen) == 36
    assert sum("ups_conv" in k for k in seen) == 12
    assert sum("narrow_conv" in k for k in seen) == 1


@needs_objects
def test_everything_else_is_refused_with_no_runtime_call(trows_calls):
    bad = [c for c in trows_calls if ".bad" in c[0]]
    assert len(bad) >= 25
    for label, rc, kernels, other in bad:
        assert rc == -1 and not kernels and not other, (label, rc, kernels, other)  # STZS_EINVAL, nothing recorded
    labels = " | ".join(c[0] for c in bad)
    for must in ("mfma snake", "lane16", "x3frag", "splitk", "mul 2", "rows 2", "trio", "pro_part", "frag32 blk leaky",
                 "ks 1 shortcut", "acc no res", "glds", "stride 2"):
        assert must in labels, must
