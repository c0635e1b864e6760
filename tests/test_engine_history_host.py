"""tests/engine_history.py without a device: engines on "cpu" over the recording stand-in of tools/launch_trace.py
(nothing is launched; the buffers are requested, sized and classified exactly as on the device).  One uniform, one
ragged, one streaming and one chunked case on the spec of tests/test_gpu_engine_history.py, and the uniform case on an
fp8-denoiser engine (the only fp8 act() buffers):

  * track() saw every key the case requested;
  * dirty() changed no integer or byte storage, no padding column, nothing outside an act() buffer's current view, no
    "keep" buffer, no non-tuple key of _bufs and nothing in _consts;
  * dirty() left every zero=False float storage NaN over its whole capacity and the data columns of every act() buffer
    at the fill value (the state is asserted, not a difference: torch.empty may hand back an earlier run's poison);
  * the classification is the same on two runs, and the case still enqueues after dirty()."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import engine_history as H  # noqa: E402

CASES = [("bf16", "U"), ("bf16", "Ra"), ("bf16", "Sr"), ("bf16", "Scu"), ("fp8", "U")]
INT_KEYS = {"text_lens", "ref_lens", "pr.idx", "pr.total", "pr.dur", "prompt.idx", "gen.frame_rows"}


@pytest.fixture(scope="module")
def spec(tiny):
    return tiny.replace(dec_out=128, gen_ch=(256, 128))


@pytest.fixture(scope="module")
def params(spec):
    from stzs.params import init_params
    return init_params(spec, seed=2)


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8).clone()


def _snapshot(eng):
    bufs = {k: _bytes(e[0] if isinstance(k, tuple) else e) for k, e in eng._bufs.items()}
    return bufs, {k: _bytes(v) for k, v in eng._consts.items()}


def _run(spec, params, kind, name):
    """the case on a fresh tracked engine, dirty(), the case again -> (classification, checks made per kind)"""
    import launch_trace as LT
    from stzs.engine import StyleTTSZS
    with LT._Patched() as lib:
        eng = StyleTTSZS(spec, params, device="cpu", fp8_denoiser=kind == "fp8")
        H.track(eng, kind)
        call = H.make_calls(spec, check=False)[name]
        n0 = len(lib.calls)
        H.run(eng, call)
        n_calls = len(lib.calls) - n0
        tup = [k for k in eng._bufs if isinstance(k, tuple)]
        assert tup and set(tup) == set(eng._history), set(tup) ^ set(eng._history)  # track() saw every request
        before, consts = _snapshot(eng)
        kinds = H.dirty(eng)
        after, consts2 = _snapshot(eng)
        assert set(kinds) == set(eng._bufs) and list(before) == list(after)
        seen = dict.fromkeys(("nan", "act", "keep", "int", "pool"), 0)
        for k, kind_k in kinds.items():
            seen[kind_k] += 1
            if kind_k in ("int", "pool", "keep"):
                assert torch.equal(before[k], after[k]), (k, kind_k)
                assert (kind_k == "pool") == (not isinstance(k, tuple))
                continue
            store, shape, view, _ = eng._bufs[k]
            assert store.dtype.is_floating_point
            if kind_k == "nan":
                assert not eng._history[k]["zero"]
                assert bool(torch.isnan(store.float()).all()), k  # the whole capacity, not only the view
                continue
            B, T_, C = eng._history[k]["act"]
            fill = H.FILL[store.dtype]
            assert eng._history[k]["zero"] and shape == (B, T_, H._rup8(C))
            assert bool((view[:, :, :C].float() == fill).all()), k
            # the padding columns and the storage past the current view: byte for byte as they were
            es, n = store.element_size(), view.numel()
            b3 = before[k][:n * es].view(B, T_, H._rup8(C) * es)
            a3 = after[k][:n * es].view(B, T_, H._rup8(C) * es)
            assert torch.equal(b3[:, :, C * es:], a3[:, :, C * es:]), k
            assert torch.equal(before[k][n * es:], after[k][n * es:]), k
            assert not bool(view[:, :, C:].float().any()), k  # (and they are the zeros the engine relies on)
        for k in consts:
            assert torch.equal(consts[k], consts2[k]), k
        for key in INT_KEYS & {k[0] for k in tup}:
            assert all(kinds[k] == "int" for k in tup if k[0] == key), key
        assert all(kinds[k] == "int" for k in tup if k[0].startswith(("lstm.xchg", "lstm.sync")))
        assert any(k[0].startswith("lstm.sync") for k in tup)
        H.run(eng, call)  # the same launches over the poisoned cache
        assert len(lib.calls) - n0 == 2 * n_calls
        assert set(k for k in eng._bufs if isinstance(k, tuple)) == set(tup)
    return {str(k): v for k, v in kinds.items()}, seen


@pytest.mark.parametrize("kind,name", CASES, ids=[f"{k}-{n}" for k, n in CASES])
def test_track_and_dirty(spec, params, kind, name):
    kinds, seen = _run(spec, params, kind, name)
    kinds2, seen2 = _run(spec, params, kind, name)
    assert kinds == kinds2 and seen == seen2  # the classification is a function of the case
    print(kind, name, seen)
    assert seen["nan"] and seen["act"] and seen["int"] and seen["pool"] and seen["keep"]  # (gen.har is "keep")
    if kind == "fp8":
        assert any(v == "act" and "float8" in k for k, v in kinds.items())
    if name == "Scu":
        assert kinds[str(("gen.har_w", torch.bfloat16))] == "keep"
        assert kinds[str(("dec.F0w", torch.float32))] == "nan"  # (the uniform chunked decoder asks for it zero=False)
    if name == "Sr":
        assert kinds[str(("gen.tail0", torch.float32))] == "nan"
        assert kinds[str(("gen.wav_stream", torch.float32))] == "nan"


def test_twin_gets_wrappers_of_its_own(spec, params):
    import launch_trace as LT
    from stzs.engine import StyleTTSZS
    with LT._Patched():
        eng = StyleTTSZS(spec, params, device="cpu")
        H.track(eng, "bf16")
        assert H.track(eng) is eng._history  # idempotent
        t = H.twin(eng)
        H.run(t, H.make_calls(spec, check=False)["U"])
        assert not eng._bufs and not eng._history and t._bufs and t._history_name == "bf16"
        assert set(k for k in t._bufs if isinstance(k, tuple)) == set(t._history)
        assert t._last_trace and "har" in t._last_trace and "post" in t._last_trace
    for fn in ("buf", "act", "decode"):  # the class keeps its own methods
        assert getattr(StyleTTSZS, fn).__qualname__ == "StyleTTSZS." + fn


def test_first_diff_names_row_sample_and_frame():
    a = torch.zeros(2, 1800)
    b = a.clone()
    assert H.first_diff(a, b, 600, "Ra", "Rb").endswith("equal")
    b[1, 1300] = 1.0
    msg = H.first_diff(a, b, 600, "Ra", "Rb", stage="stage har: row 1")
    assert "call Ra after Rb" in msg and "row 1 sample 1300 (40-fps frame 2)" in msg and "1 of 3600" in msg
    assert msg.endswith("stage har: row 1")
    assert "fresh engine gives (2, 1800)" in H.first_diff(a[:, :5], b, 600)
    b[1, 1300] = float("nan")
    assert "row 1 sample 1300" in H.first_diff(a, b, 600)
