"""The native dispatch, checked without a device (tools/dispatch_trace.py): the library's objects linked against the
recording runtime stand-in (tools/hip_record/hip_record.cpp) run their real validation and routing on fake pointers,
and every launch is recorded.  Properties only -- no golden digest: a routing rule changed on purpose needs no edit
here.  The trace library is linked into a temporary directory and loaded by child processes only."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
TOOL = os.path.join(ROOT, "tools", "dispatch_trace.py")
OBJECTS = os.path.join(ROOT, "styletts-zs_amd", "build")
LDS_MAX = 160 * 1024

pytestmark = pytest.mark.skipif(
    shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h") or
    not os.path.exists(os.path.join(OBJECTS, "dispatch.o")),
    reason="needs g++, the HIP headers and the library's objects (styletts-zs_amd/build.py)")


def _run(tmp, *args):
    r = subprocess.run([sys.executable, TOOL, "--lib", str(tmp / "libstzs_trace.so")] + [str(a) for a in args],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dispatch_trace")
    for n in ("a", "b"):
        _run(tmp, "--sweep", "--out", tmp / f"sweep_{n}.txt")
    return tmp / "sweep_a.txt", tmp / "sweep_b.txt"


def test_sweep_accepted_calls_launch_rejected_calls_do_not(sweeps):
    """every accepted call launches (non-zero grid and block, LDS within the CU's 160 KB); a rejected stzs_conv1d /
    stzs_ln_linear call makes no runtime call at all -- stzs.h's "validates before any HIP call" over the whole
    sweep; a rejected group has launched at most the problems before the failing one (two kernels each at most)"""
    import dispatch_trace as D
    entries = D.parse(sweeps[0])
    assert len(entries) > 5000
    accepted = rejected = 0
    for kind, label, rc, lines in entries:
        assert kind == "call" and rc is not None, label
        if rc < 0:
            rejected += 1
            # (stzs_conv1d_group returns the first failing problem's code: "the problems before it have been launched")
            if label.startswith("stzs_conv1d_group"):
                assert sum(ln.startswith("L ") for ln in lines) <= 2 * 2, (label, rc, lines)
            else:
                assert not lines, (label, rc, lines[:3])
            continue
        accepted += 1
        launches = [ln.split() for ln in lines if ln.startswith("L ")]
        assert launches, (label, rc)
        for ln in launches:
            assert ln[1] != "?", (label, ln)  # (a registered kernel)
            assert all(int(v) > 0 for v in ln[2:8]) and 0 <= int(ln[8]) <= LDS_MAX, (label, ln)
        for ln in lines:
            if ln.startswith("A "):
                assert 0 < int(ln.split()[3]) <= LDS_MAX, (label, ln)
    assert accepted > 1000 and rejected > 1000, (accepted, rejected)


def test_sweep_deterministic(sweeps):
    assert open(sweeps[0]).read() == open(sweeps[1]).read()


def test_synth_trace_matches_engine_launch_count(tmp_path):
    """the eight cases at the tiny spec through the real dispatch: the engine's launch count is the number of library
    calls that launched (a group call counting as its return value), and no case launches fewer kernels than that"""
    out = _run(tmp_path, "--synth", "tiny", "--out", tmp_path / "synth.txt")
    rows = [dict(f.split("=") for f in ln.split()[1:]) for ln in out.splitlines() if "engine.launches=" in ln]
    assert len(rows) == 8, out
    for r in rows:
        assert int(r["engine.launches"]) == int(r["launching_calls"]) > 0, r
        assert int(r["kernels"]) >= int(r["launching_calls"]), r
    assert "L ? " not in open(tmp_path / "synth.txt").read()


def test_linear_probe_cases_launch_what_the_gpu_test_claims(tmp_path):
    """the identity-probe table of tests/test_gpu_linear_probe.py (refops.linear_cases) through the engine's routing and
    the real dispatch: each case launches exactly one kernel of the family it names -- gemm_glds 64-row against 128-row
    told apart by grid.x and the LDS bytes, gemm_rows / rows16 by name -- with the grid refops.lin_expected_launch
    restates and grid.z = its K slices.  The stand-in reports 256 CUs, so refops.gemm_tile_rows (the launcher's tile
    rule, restated for the GPU test) is compared with the launcher's own choice on every gemm_glds case."""
    import dispatch_trace as D
    import refops as R
    _run(tmp_path, "--linear-cases", "--out", tmp_path / "lin.txt")
    entries = {label: (rc, lines) for _, label, rc, lines in D.parse(tmp_path / "lin.txt")}
    cases = R.linear_cases(256)
    assert len(entries) == len(cases) > 100
    assert any(c.kern == "glds128" for c in cases), "no 128-row-tile case at 256 CUs"
    lds = {}
    for c in cases:
        rc, lines = entries[R.lin_id(c)]
        launches = [ln.split() for ln in lines if ln.startswith("L ")]
        assert rc == 0 and len(launches) == 1, (R.lin_id(c), rc, lines)
        name, grid, nlds = launches[0][1], tuple(int(v) for v in launches[0][2:5]), int(launches[0][8])
        want, gx, gy, gz = R.lin_expected_launch(c)
        assert want in name and sum(k in name for k in ("gemm_glds", "gemm_rows", "rows16", "ln_rows")) == 1, (R.lin_id(c), name)
        assert grid == (gx, gy, gz), (R.lin_id(c), grid, (gx, gy, gz))
        if want == "gemm_glds":
            tile = 64 if c.Z > 1 else R.gemm_tile_rows(c.B * c.T, (c.Co + 127) // 128 * 128, 256)
            assert tile == (128 if c.kern == "glds128" else 64), R.lin_id(c)
            lds.setdefault(tile, set()).add(nlds)
        else:
            assert nlds <= 16 * 1024, (R.lin_id(c), nlds)  # (static LDS only)
    assert len(lds[64]) == len(lds[128]) == 1 and max(lds[64]) < min(lds[128]) <= LDS_MAX, lds


def test_precise_probe_cases_launch_what_the_gpu_test_claims(tmp_path):
    """every launch of tests/test_gpu_precise_probe.py (refops.precise_probe_cases / precise_exact_cases /
    precise_dense_cases) through the engine's routing and the real dispatch: each is accepted and launches exactly one
    kernel of the family it names (mrfx_conv / mrfx_lin / conv_x3), with the grid and the dynamic LDS bytes of
    refops.px_expected_launch -- 2 rows_in 256 + 2048 tells the 128-row tile from the 64-row tile, the template arguments
    in the kernel's name the tap count and tile height; conv_x3: refops.x3_lds_bytes tells the padded row pitch from the
    tight one (the stride-6 conv: 148 608 B), the name the prologue instantiation and the FLAT form.  k7 d5 runs 128-row tiles (158 staged rows, 82 944 B of LDS: one
    workgroup per CU); the k3 and k7 instantiations of the 64-row form are never launched."""
    import dispatch_trace as D
    import refops as R
    _run(tmp_path, "--precise-cases", "--out", tmp_path / "px.txt")
    entries = {label: (rc, lines) for _, label, rc, lines in D.parse(tmp_path / "px.txt")}
    want = {}
    for c in R.precise_probe_cases():
        want[f"probe {R.px_id(c)}"] = want[f"probe.compact {R.px_id(c)}"] = c
    for v in R.precise_exact_cases():
        want[f"exact {R.px_exact_id(v)}"] = v[0]
    for v in R.precise_dense_cases():
        want[f"dense {R.px_dense_id(v)}"] = v[0]
    assert set(entries) == set(want) and len(want) > 150
    seen = set()
    for label, c in want.items():
        rc, lines = entries[label]
        launches = [ln.split() for ln in lines if ln.startswith("L ")]
        assert rc == 0 and len(launches) == 1, (label, rc, lines)
        name, grid, nlds = launches[0][1], tuple(int(v) for v in launches[0][2:5]), int(launches[0][8])
        kern, gx, gy, lds = R.px_expected_launch(c)
        assert kern in name and sum(k in name for k in ("mrfx_lin", "mrfx_conv", "conv_x3")) == 1, (label, name)
        assert grid == (gx, gy, 1) and nlds == lds <= LDS_MAX, (label, grid, nlds, (gx, gy, lds))
        if kern == "mrfx_conv":  # mrfx_conv<PACT, HR, HA, KS, BT, NCH, AL, NW>
            targs = name.split("mrfx_convI")[1].split("EEEv")[0].split("E")
            ks, bt, nch, nw = int(targs[3][2:]), int(targs[4][2:]), int(targs[5][2:]), targs[7] == "Lb1"
            assert (ks, bt, nw) == (c.k, c.tile, c.kern == "narrow"), (label, name)
            assert nch == (1 if c.Ci <= 128 and R.PX_PRO[c.pro][1] == "snake" or nw else 0), (label, name)
            seen.add((ks, bt))
        if kern == "conv_x3":  # conv_x3<float, float, PACT, FLAT>
            targs = name.split("conv_x3I")[1].split("EEEv")[0]
            pact = {None: 0, "leaky": 1, "snake": 2}[R.PX_PRO[c.pro][1]]
            assert targs == f"ffLi{pact}ELb{int(c.kern == 'x3flat')}", (label, name)
            seen.add(("x3", pact, c.kern == "x3flat", nlds))
    assert {v for v in seen if v[0] != "x3"} == {(3, 128), (7, 128), (11, 128), (11, 64)}, seen
    assert {v[1:3] for v in seen if v[0] == "x3"} == {(0, False), (1, False), (2, False), (0, True)}, seen
    assert {v[3] for v in seen if v[0] == "x3"} == {R.x3_lds_bytes(129), R.x3_lds_bytes(774)} == {76800, 148608}
    k7d5 = R.px_expected_launch(R.PxCase("conv", 2, 300, 128, 128, 7, 5, "snake", 128))
    assert k7d5[3] == 82944 and 2 * k7d5[3] > LDS_MAX
