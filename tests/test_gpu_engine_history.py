"""The result of a call must not depend on what ran on the engine before (the buffer contract): every
public synthesis mode is held to the bits a FRESH engine gives -- a twin on the same packed weights with an empty
buffer cache -- after (a) tests/engine_history.py dirty() has poisoned the engine's own cached buffers within the
contract, (b) a real predecessor at the same padded shape left stale activations and stale (in-range) lengths, indices
and sync words, (c) a seeded session of all calls, (d) graph replays interleaved with eager calls.

Engines: D the default bf16 engine on SPEC_TINY with dec_out 128 and gen_ch (256, 128) (the spec of
tests/test_gpu_ragged_decoder_stages.py), P precise=True precise_frontend=True on the same spec, L the latency engine on
SPEC_TINY (uniform rows only: its refusal of ragged frames is asserted once).  D and P: B = 4, T = 12, references of
sr / 2 samples; L: B = 1.  The calls (engine_history.make_calls):

    U   uniform synth, forced 7 frames per row            Sw  synth_stream, whole decoder + streaming iSTFT, uniform,
    Rt  ragged text + ragged references, 7 frames each        chunks of 2 frames: 2 + 2 + 2 + 1
    Ra  ragged_frames, forced [7, 1, 3, 6]                 Sr  the same, ragged_frames, frames of Ra
    Rb  ragged_frames, forced [1, 7, 6, 3]                 Sc  synth_stream(chunked_halo=1), ragged
    Rp  ragged_frames, predicted, ragged text + refs       X   synth(ref_sr=16000, out_sr=22050, int16), ragged
    C   row_controls (guidance, speed, pitch), ragged      A   Sr abandoned after its first chunk (leaves state only)
    U2  U at double amplitude; Us / Ul: a smaller / a larger uniform shape (the graph test)

Every comparison is torch.equal on host copies; where the design promises zeros (the waveform past 600 frame_lens[b]
or its out_sr image, har rows past the row's own frames) they are checked too -- over buffers that were not zero before.
check_status() is 0 after every call (engine_history.run).

Does the file see a defect the older stage tests do not?  Three value-only mutations of ragged tails on the device
(none changes an address), tests/test_gpu_ragged_decoder_stages.py ("old", 5 tests) and this file (63), each run once:
  * csrc/mrfv_kernel.hpp, the staging zero mask of the ragged forms testing `tin < a.T_in` instead of `tin < Tin` (the
    load still clamps into the row): old 3 failed / 2 passed, this file 63 passed.  The staged value is then the
    transformed row T_b - 1 -- the row's own data, so a fresh engine with the same kernel computes the same wrong bits:
    a defect that does not depend on the history is the row-against-solo tests' to find, and they do.
  * csrc/istft.hip, the zero store for the samples past a row's own last one skipped (`if (m >= m_end) continue;`):
    old 1 failed (its graph test zeroes the output before the replay; the row-against-solo tests run on a fresh
    torch.empty waveform and pass) / 4 passed, this file 42 failed / 21 passed -- every ragged call behind dirty() or
    behind a longer row "differs from a fresh engine" in its tail (stale samples or dirty()'s NaN).
  * csrc/source.hip, the zero store of the har frames past a row's own Tf_b skipped: old 5 passed -- its ragged call is
    the first at its shape, the buffer is freshly zeroed, and "har rows past its own frames are zeros" holds whatever
    the kernel does -- this file 33 failed / 30 passed, e.g. "call D:Ra after U: differs from a fresh engine in 6000 of
    16800 samples, first at row 1 sample 0 (40-fps frame 0) ...; stage mrf_in0: row 1 differs first at its row 19 of 20
    valid" (the noise conv reads the stale har rows as its padding).
None faulted; none is committed.  On the unmutated library all 63 pass: no defect found.  Wall time of the module on
an MI355X: 2.3 s (4.5 s with start-up), the slowest test 0.8 s."""
import random
import time

import pytest
import torch

import engine_history as H

pytestmark = pytest.mark.gpu

FULL = ["U", "Rt", "Ra", "Rb", "Rp", "C", "Sw", "Sr", "Sc", "X"]
UNIFORM = ["U", "Sw"]
PAIRS = [("Ra", "Rb"), ("Rb", "Ra"), ("U", "Ra"), ("Ra", "U"), ("Rt", "U"), ("U", "Rt"), ("C", "Ra"), ("Ra", "C"),
         ("Sw", "Sr"), ("Sr", "Sw"), ("A", "Sr"), ("A", "Sw"), ("Sc", "Ra"), ("Ra", "Sc"), ("X", "Ra"), ("U2", "U")]
CASES = [(e, c) for e in ("D", "P") for c in FULL] + [("L", c) for c in UNIFORM]
PAIR_CASES = [(e, p) for e in ("D", "P") for p in PAIRS] + [("L", ("U2", "U"))]


@pytest.fixture(scope="module")
def spec(tiny):
    return tiny.replace(dec_out=128, gen_ch=(256, 128))


@pytest.fixture(scope="module")
def wall():
    t0 = time.time()
    yield
    print(f"\ntests/test_gpu_engine_history.py: {time.time() - t0:.1f} s wall, {len(H._FRESH)} fresh references")


@pytest.fixture(scope="module")
def engines(gpu_device, spec, tiny, tiny_params, wall):
    """-> {name: (engine, spec, calls)}"""
    from stzs.engine import StyleTTSZS, latency_engine
    from stzs.params import init_params
    P = init_params(spec, seed=2)
    d = StyleTTSZS(spec, P, device=gpu_device)
    p = StyleTTSZS(spec, P, device=gpu_device, precise=True, precise_frontend=True)
    for e in (d, p):
        e._check_ragged_decoder()
    lat = latency_engine(tiny, StyleTTSZS(tiny, tiny_params, device=gpu_device).W, gpu_device)
    out = {"D": (d, spec, H.make_calls(spec)), "P": (p, spec, H.make_calls(spec)),
           "L": (lat, tiny, H.make_calls(tiny, B=1))}
    for name, (e, _, _) in out.items():
        H.track(e, name)
    return out


def _tail_start(S, call, n):
    """first sample past a row of n 40-fps frames in the call's output"""
    if call.out_sr is None:
        return S.frame40 * n
    from stzs.resample import out_len, ratio
    return out_len(S.frame40 * n, *ratio(S.sr, call.out_sr))


def _same(eng, S, call, got, pred=""):
    """got (engine_history.run) against the fresh engine's result, and the zeros the design promises"""
    want = H.fresh(eng, call)
    gw, ww = got["wav"], want["wav"]
    assert bool(ww.any()) and (not ww.is_floating_point() or bool(torch.isfinite(ww).all()))
    if gw.shape != ww.shape or gw.dtype != ww.dtype or not torch.equal(gw, ww):
        f40 = S.frame40 if call.out_sr is None else S.frame40 * call.out_sr / S.sr
        stage = H.first_stage_diff(S, H.host_trace(eng), want["trace"], want["fl"])
        pytest.fail(H.first_diff(gw, ww, f40, f"{eng._history_name}:{call.name}", pred, stage))
    assert got["fl"] == want["fl"] and got["spans"] == want["spans"], (call.name, pred, got["fl"], got["spans"])
    if got["fl"] is not None:
        for b, n in enumerate(got["fl"]):
            assert not bool(gw[b, _tail_start(S, call, n):].any()), \
                f"{call.name} after {pred}: row {b} ({n} frames): the waveform tail is not exact zeros"
    if want["har"] is not None:
        gh = got["har"]
        assert torch.equal(H._bits(gh), H._bits(want["har"])), f"{call.name} after {pred}: har differs"
        for b, n in enumerate(got["fl"] or []):
            assert not bool(gh[b, H.trace_rows(S, n)["har"]:].float().any()), \
                f"{call.name} after {pred}: row {b}: har rows past its own frames are not zeros"


def test_fresh_is_deterministic(engines):
    """two twins give the same bits for every call: without this the other tests mean nothing"""
    n = 0
    for name, (eng, S, calls) in engines.items():
        for cn in (FULL + ["U2", "Us", "Ul"] if name != "L" else UNIFORM + ["U2", "Us", "Ul"]):
            t = H.twin(eng)
            _same(t, S, calls[cn], H.run(t, calls[cn]), "nothing (a second fresh engine)")
            n += 1
        # (and they are different results: equal bits are not the equality of constants)
        w = {cn: H.fresh(eng, calls[cn])["wav"] for cn in (("U", "U2") if name == "L" else ("U", "U2", "Ra", "Rb"))}
        assert not torch.equal(w["U"], w["U2"]) and (name == "L" or not torch.equal(w["Ra"], w["Rb"]))
    print("fresh references", n)


def test_latency_engine_refuses_ragged_frames(engines):
    """the only cases left out: the latency engine's ragged ones, refused by design before any launch"""
    eng, S, calls = engines["L"]
    d = calls.data
    n0 = eng.launches
    kw = dict(steps=H.STEPS, cfg_scale=H.CFG, noise=d["eps"], durations=d["dur7"], seeds=[3], ragged_frames=True)
    with pytest.raises(NotImplementedError):
        eng.synth(d["tok"], d["ref"], **kw)
    with pytest.raises(NotImplementedError):
        next(eng.synth_stream(d["tok"], d["ref"], **kw))
    assert eng.launches == n0


@pytest.mark.parametrize("name,cn", CASES, ids=[f"{e}-{c}" for e, c in CASES])
def test_dirty_buffers(engines, name, cn):
    """warm the engine at the call's shapes, poison its cached buffers, make the call"""
    eng, S, calls = engines[name]
    call = calls[cn]
    _same(eng, S, call, H.run(eng, call), "whatever ran before (warm-up)")
    kinds = H.dirty(eng)
    assert "nan" in kinds.values() and "act" in kinds.values()
    _same(eng, S, call, H.run(eng, call), "itself + dirty()")


@pytest.mark.parametrize("name,pair", PAIR_CASES, ids=[f"{e}-{a}-{b}" for e, (a, b) in PAIR_CASES])
def test_same_shape_successor(engines, name, pair):
    """what a scheduler bucket does: the call right behind a real predecessor at the same padded shape, no dirty()"""
    eng, S, calls = engines[name]
    pred, call = calls[pair[0]], calls[pair[1]]
    got = H.run(eng, pred)
    if got is not None:
        _same(eng, S, pred, got, "whatever ran before")
    _same(eng, S, call, H.run(eng, call), pred.name)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("name", ["D", "P"])
def test_session(engines, name, seed):
    """all calls of the table in a fixed seeded order on one engine, dirty() before every second call"""
    eng, S, calls = engines[name]
    order = FULL + ["A"]
    random.Random(seed).shuffle(order)
    print(name, seed, order)
    pred = "the tests before"
    for i, cn in enumerate(order):
        if i % 2:
            H.dirty(eng)
            pred += " + dirty()"
        got = H.run(eng, calls[cn])
        if got is not None:
            _same(eng, S, calls[cn], got, pred)
        pred = cn


@pytest.mark.parametrize("name", ["D", "L"])
def test_graph_replay_between_eager_calls(engines, name):
    """capture synth() for U and replay it; an eager call at the same shapes (Ra; U2 on the latency engine), one at a
    smaller and one at a larger shape (it grows the storages; the captured ones are retired, not freed); replay again"""
    base, S, calls = engines[name]
    eng = H.twin(base)  # (a buffer cache of its own: a capture pins its shapes)
    dev = eng.device
    d = calls.data
    B = d["tok"].shape[0]
    tok, ref, eps, dur = d["tok"].to(dev, torch.int32), d["ref"].to(dev), d["eps"].to(dev), d["dur7"].to(dev)

    def fn():
        return eng.synth(tok, ref, steps=H.STEPS, cfg_scale=H.CFG, noise=eps, durations=dur, seeds=H.SEEDS[:B],
                         n_frames=7, check=False)["wav"]

    want = H.fresh(base, calls["U"])["wav"]
    graph, out = eng.capture(fn)

    def replay(when):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert graph.check() == 0
        got = out.cpu().clone()
        assert torch.equal(got, want), H.first_diff(got, want, S.frame40, f"{name}:replay of U", when)

    replay("its capture")
    pred = "a replay of U"
    for cn in ("Ra" if name == "D" else "U2", "Us", "Ul", "U"):
        _same(eng, S, calls[cn], H.run(eng, calls[cn]), pred)
        pred = cn
    assert eng._retired, "the larger call should have retired the captured storages"
    replay("eager Ra / U2, Us, Ul, U")
