"""Per-row lengths on the precise engines, the host side -- no GPU: the dispatch of every launch shape of
tests/test_gpu_ragged_precise_kernels.py (tools/dispatch_trace.py --ragged-precise-cases: the real host dispatch of this
build linked with the recording runtime stand-in) and the acceptance / refusal matrix of _check_ragged_frames() /
_check_ragged_decoder() over engines' weights packed on "cpu"."""
import os
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "dispatch_trace.py")
OBJECTS = os.path.join(ROOT, "styletts-zs_amd", "build")
sys.path.insert(0, os.path.join(ROOT, "tools"))

needs_objects = pytest.mark.skipif(
    shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h") or
    not os.path.exists(os.path.join(OBJECTS, "dispatch.o")),
    reason="needs g++, the HIP headers and the library's objects (styletts-zs_amd/build.py)")


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    """{"rag" | "uni" | "bad": {label: (return code, [(kernel, grid, block, lds)], other runtime lines)}}"""
    import dispatch_trace as D
    tmp = tmp_path_factory.mktemp("ragx")
    r = subprocess.run([sys.executable, TOOL, "--lib", str(tmp / "libstzs_trace.so"), "--ragged-precise-cases", "--out",
                        str(tmp / "t.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {"rag": {}, "uni": {}, "bad": {}}
    for kind, text, rc, lines in D.parse(tmp / "t.txt"):
        k, label = text.split(" ", 1)
        launches = []
        for ln in lines:
            if ln.startswith("L "):
                f = ln.split()
                launches.append((f[1], tuple(f[2:5]), tuple(f[5:8]), f[8]))
        out[k][label] = (rc, launches, [ln for ln in lines if not ln.startswith("L ") and not ln.startswith("A ")])
    return out


@needs_objects
def test_every_accepted_case_launches_the_rag_instance_of_its_sibling(trace):
    """with lengths: one launch of the kernel whose trailing template argument (RAG) is true, with the grid, block and LDS
    bytes of the same problem without lengths"""
    import ragged_precise_cases as RP
    acc = RP.accepted()
    assert len(acc) >= 100 and set(trace["rag"]) == set(trace["uni"]) == {c["label"] for c in acc}
    seen = set()
    for c in acc:
        rc, ls, other = trace["rag"][c["label"]]
        rc0, ls0, _ = trace["uni"][c["label"]]
        assert rc == rc0 == 0 and len(ls) == len(ls0) == 1 and not other, (c["label"], rc, rc0, ls, ls0, other)
        (k, grid, block, lds), (k0, grid0, block0, lds0) = ls[0], ls0[0]
        if c["form"] == "fx3":  # mrfx_conv<..., NW, RAG>: the sibling is the same instance with RAG = false
            assert "mrfx_convI" in k and k.endswith("Lb1EEEv14stzs_conv_args"), (c["label"], k)
            assert k0 == k[:-len("Lb1EEEv14stzs_conv_args")] + "Lb0EEEv14stzs_conv_args", (c["label"], k, k0)
        else:  # conv_x3<float, float, X3_RAG (8) | act, false> beside conv_x3<float, float, act, false>
            pact = {"none": 0, "leaky": 1, "snake": 2}[c["act"]]
            assert k.split("conv_x3I")[1].split("EEEv")[0] == f"ffLi{8 + pact}ELb0", (c["label"], k)
            assert k0.split("conv_x3I")[1].split("EEEv")[0] == f"ffLi{pact}ELb0", (c["label"], k0)
        assert (grid, block, lds) == (grid0, block0, lds0), (c["label"], ls, ls0)
        seen.add(k)
    # mrfx: Snake (4 epilogues x (k3, k7, k11 at 128-row tiles + k11 at 64-row tiles) x single- / multi-chunk) + the narrow
    # conv_post form + the 4 block forms; conv_x3: one instance per prologue activation
    assert sum("mrfx_conv" in k for k in seen) == 4 * 4 * 2 + 1 + 4
    assert sum("conv_x3" in k for k in seen) == 3


@needs_objects
def test_every_refusal_returns_einval_with_no_runtime_call(trace):
    import ragged_precise_cases as RP
    bad = RP.refused()
    assert len(bad) >= 12 and set(trace["bad"]) == {c["label"] for c in bad}
    for c in bad:
        rc, ls, other = trace["bad"][c["label"]]
        assert rc == c["want"] == -1 and not ls and not other, (c["label"], rc, ls, other)
    labels = " | ".join(c["label"] for c in bad)
    for must in ("fx3.flat linear", "x3.flat linear", "fx3.snake bf16 rows", "stride 2", "acc no res", "rows 1 mul 2"):
        assert must in labels, must


@needs_objects
def test_without_lengths_nothing_is_rerouted(trace):
    """the same table with t_lens = NULL launches only kernels without RAG -- the instances the build had before"""
    for label, (rc, ls, _) in trace["uni"].items():
        k = ls[0][0] if len(ls) == 1 else ""
        assert rc == 0 and k.endswith("Lb0EEEv14stzs_conv_args"), (label, ls)
        assert "mrfx_convI" in k or k.split("conv_x3I")[1].split("EEEv")[0] in ("ffLi0ELb0", "ffLi1ELb0", "ffLi2ELb0"), (label, k)


# ---- the engines' checks ---------------------------------------------------------------------------------------------

def _engine(spec, precise=False, precise_decoder=False, fp8_denoiser=False):
    """an engine object with the attributes the two checks read and the weights its constructor would pack (host tensors,
    not filled): no device, no library"""
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.weights import PackedModel
    e = StyleTTSZS.__new__(StyleTTSZS)
    pd = precise_decoder or precise
    e.blk_splitk, e.precise, e.precise_all, e.launches = 0, pd, precise, 0
    e.dec_dt = torch.float32 if pd else torch.bfloat16
    e.W = PackedModel(spec, init_params(spec, seed=0), torch.device("cpu"), fill=False, precise=pd, precise_all=precise,
                      lowp_denoiser=fp8_denoiser)
    return e


@pytest.fixture(scope="module")
def spec128(tiny):
    return tiny.replace(dec_out=128, gen_ch=(256, 128))


@pytest.mark.parametrize("kw", [dict(precise=True), dict(precise_decoder=True), dict(precise=True, fp8_denoiser=True), dict()],
                         ids=["precise", "precise_decoder", "precise_fp8", "default"])
def test_engines_that_take_the_lengths(kw, spec128):
    from stzs.scheduler import BucketScheduler
    e = _engine(spec128, **kw)
    e._check_ragged_frames()
    e._check_ragged_decoder()
    sch = BucketScheduler(e, ragged_text=True, ragged_ref=True, ragged_frames=True, ragged_decoder=True)
    assert sch.ragged_frames and sch.ragged_decoder and e.launches == 0


@pytest.mark.parametrize("kw", [dict(precise=True), dict(precise_decoder=True)], ids=["precise", "precise_decoder"])
def test_precise_engines_on_spec_tiny(kw, tiny):
    """a precise decoder's convs all have split-operand weights -> conv_x3 / mrfx whatever the spec's widths"""
    e = _engine(tiny, **kw)
    e._check_ragged_frames()
    e._check_ragged_decoder()


def test_still_refused(tiny, spec128):
    from stzs.scheduler import BucketScheduler
    # the latency engine's split-K blocks: frames and decoder, whatever the decoder's precision
    for kw in (dict(), dict(precise=True)):
        e = _engine(spec128, **kw)
        e.blk_splitk = 4
        for chk in (e._check_ragged_frames, e._check_ragged_decoder,
                    lambda: BucketScheduler(e, ragged_frames=True, ragged_decoder=True)):
            with pytest.raises(NotImplementedError, match="blk_splitk"):
                chk()
    # SPEC_TINY's generic-path bf16 generator convs
    e = _engine(tiny)
    e._check_ragged_frames()
    with pytest.raises(NotImplementedError, match="generic-path bf16"):
        e._check_ragged_decoder()
    # an fp32 decoder whose convs have no split-operand weights (they would run on conv_f32)
    e = _engine(spec128)
    e.dec_dt = torch.float32
    with pytest.raises(NotImplementedError, match="conv_f32"):
        e._check_ragged_decoder()
    assert e.launches == 0
