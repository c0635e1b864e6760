"""Per-request controls through the engine, SPEC_TINY, the inputs of
tests/test_gpu_ragged_frames_stages._inputs (B 4, T 12, seed 99): guidance scales [5, 1, 2.5, 0], speaking rates
[1, 0.5, 1.7, 4.0] (frame counts [48, 96, 24, 12], tests/test_refops_controls.py), pitch shifts [0, 12, -7, 3.5].

Row b of a batch run with controls must compute what the engine computes for that row alone with its values given as
scalars: max-abs <= 1e-6 of max|ref| (the ragged tests' bound; bit-identical is expected and which one held is
printed).  Against the oracle: the style codes and F0 / N at the bounds of tests/test_gpu_stages.py, the durations equal
outside a tie guard on the quotients dsum / r_b -- which must excuse no token on these inputs.  Neutral controls are the
call without them, bit for bit and launch for launch.  A graph captured once replays with what RowControls.set()
wrote.  On the ragged decoder's spec, synth(controls=..., ragged_frames=True) gives every row its solo waveform."""
import pytest
import torch

import refops_controls as RC
from refops import rel_err
from test_gpu_ragged_frames_stages import B, T, _h_act, _host, _inputs, _near

pytestmark = pytest.mark.gpu

SCALES = [5.0, 1.0, 2.5, 0.0]
RATES = [1.0, 0.5, 1.7, 4.0]
SHIFTS = [0.0, 12.0, -7.0, 3.5]
FRAMES = [48, 96, 24, 12]
STEPS = 2


def _sampler_inputs(S):
    g = torch.Generator().manual_seed(199)
    prompt = torch.randn(B, S.L_s, S.code_dim, generator=g) * 0.3
    eps = torch.randn(B, S.L_s, S.code_dim, generator=g)
    return prompt, eps


@pytest.fixture(scope="module")
def eng(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    return StyleTTSZS(tiny, tiny_params, device=gpu_device)


@pytest.fixture(scope="module")
def engines(eng, gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS, latency_engine
    return dict(default=lambda: eng, latency=lambda: latency_engine(tiny, eng.W, gpu_device),
                precise=lambda: StyleTTSZS(tiny, tiny_params, device=gpu_device, precise=True),
                fp8=lambda: StyleTTSZS(tiny, tiny_params, device=gpu_device, fp8_denoiser=True))


@pytest.mark.parametrize("kind", ["default", "latency", "precise", "fp8"])
def test_mixed_guidance_rows_match_solo(engines, tiny, tiny_params, kind):
    S = tiny
    e = engines[kind]()
    dev = e.device
    h, _ = _inputs(S)
    prompt, eps = _sampler_inputs(S)
    rc = e.row_controls(B, cfg_scale=SCALES)
    n0 = e.launches
    got = e.sample_style(_h_act(e, h), prompt.to(dev), eps.to(dev), STEPS, controls=rc).cpu().clone()
    n_rows = e.launches - n0
    n0 = e.launches
    e.sample_style(_h_act(e, h), prompt.to(dev), eps.to(dev), STEPS, 5.0)
    assert e.launches - n0 == n_rows  # the CFG form's launches, the per-row combine in the scalar one's place
    for b, s in enumerate(SCALES):
        one = e.sample_style(_h_act(e, h[b:b + 1]), prompt[b:b + 1].to(dev), eps[b:b + 1].to(dev), STEPS, s).cpu()
        _near(f"{kind} row {b} (scale {s})", got[b], one[0])
    if kind == "default":
        from oracle import stzs_ref as R
        for b, s in enumerate(SCALES):
            with torch.no_grad():
                ref = R.sample_style(tiny_params, S, h[b:b + 1], prompt[b:b + 1], eps[b:b + 1], STEPS, s)
            err = rel_err(got[b:b + 1], ref)
            print(f"  row {b} (scale {s}) against the oracle: {err:.2e}")
            assert err < 2e-2  # (tests/test_gpu_stages.py test_sample_style at 2 steps)
    # a scale of 1 everywhere, per row: the plain form, the bits and launches of cfg_scale = 1
    n0 = e.launches
    plain = e.sample_style(_h_act(e, h), prompt.to(dev), eps.to(dev), STEPS, 1.0).cpu().clone()
    n_plain = e.launches - n0
    n0 = e.launches
    ones = e.sample_style(_h_act(e, h), prompt.to(dev), eps.to(dev), STEPS, controls=e.row_controls(B, cfg_scale=[1.0] * B))
    assert e.launches - n0 == n_plain and torch.equal(ones.cpu(), plain)


_runs = {}


def _prosody(eng, S):
    """the batch with rates and shifts, the same batch unshifted, and every row alone at its own controls -- once"""
    if "pro" not in _runs:
        dev = eng.device
        h, codes = _inputs(S)
        rc = eng.row_controls(B, speed=RATES, pitch_shift=SHIFTS)
        pro = eng.predict_prosody(_h_act(eng, h), codes.to(dev), ragged_frames=True, controls=rc)
        rag = _host(S, pro, True)
        rag["dsum"] = pro["dsum"].cpu().clone()
        flat = _host(S, eng.predict_prosody(_h_act(eng, h), codes.to(dev), ragged_frames=True,
                                            controls=eng.row_controls(B, speed=RATES)), True)
        solos = []
        for b in range(B):
            one = eng.row_controls(1, speed=RATES[b], pitch_shift=SHIFTS[b])
            solos.append(_host(S, eng.predict_prosody(_h_act(eng, h[b:b + 1]), codes[b:b + 1].to(dev), controls=one), False))
        assert eng.check_status() == 0
        _runs["pro"] = (h, codes, rag, flat, solos)
    return _runs["pro"]


def test_prosody_rows_match_solo_at_their_own_controls(eng, tiny):
    _, _, rag, flat, solos = _prosody(eng, tiny)
    print("frame counts", rag["frame_lens"].tolist())
    assert rag["frame_lens"].tolist() == FRAMES and rag["T40"] == max(FRAMES)
    for b, n in enumerate(FRAMES):
        one = solos[b]
        print(f"row {b} (rate {RATES[b]}, shift {SHIFTS[b]}: {n} frames)")
        assert one["T40"] == n
        assert torch.equal(rag["dur"][b], one["dur"][0])
        assert torch.equal(rag["idx"][b, :n], one["idx"][0]) and bool((rag["idx"][b, n:] == -1).all())
        _near("en", rag["en"][b, :n], one["en"][0])
        _near("F0", rag["F0"][b, :2 * n], one["F0"][0])
        _near("N", rag["N"][b, :2 * n], one["N"][0])
        # the shift is one fp32 multiply of the unshifted curve, N is untouched
        assert torch.equal(rag["F0"][b, :2 * n], flat["F0"][b, :2 * n] * RC.pitch_factor(SHIFTS[b]))
        assert torch.equal(rag["N"][b, :2 * n], flat["N"][b, :2 * n])
    assert torch.equal(rag["dur"], flat["dur"]) and torch.equal(rag["idx"], flat["idx"])


def test_prosody_rows_match_oracle(eng, tiny, tiny_params):
    from oracle import stzs_ref as R
    S, P = tiny, tiny_params
    h, codes, rag, _, _ = _prosody(eng, S)
    with torch.no_grad():
        free = [R.predict_prosody(P, S, h[b:b + 1], codes[b:b + 1]) for b in range(B)]
    dsum_ref = torch.cat([p["dur_sum"] for p in free])
    want = RC.durations_with_rate(dsum_ref, RATES)
    assert want.sum(1).tolist() == FRAMES
    # the guard of _dur_guarded_equal on the quotients: equal wherever the oracle's quotient is farther from a rounding
    # tie than the measured error of the GPU's quotient (+ 1e-4)
    r = torch.tensor(RATES)[:, None]
    err = float((rag["dsum"] / r - dsum_ref / r).abs().max())
    ties = RC.quotient_ties(dsum_ref, RATES, err)
    print(f"quotient max abs error {err:.3e}, guarded ties {int(ties.sum())} of {ties.numel()}")
    assert bool(((rag["dur"] == want) | ties).all())
    assert int(ties.sum()) == 0  # (no quotient within 0.12 of a tie on these inputs: the guard excuses nothing)
    for b, n in enumerate(FRAMES):
        with torch.no_grad():
            pr = R.predict_prosody(P, S, h[b:b + 1], codes[b:b + 1], want[b:b + 1])
        assert torch.equal(rag["idx"][b:b + 1, :n], pr["idx"])
        eF = rel_err(rag["F0"][b:b + 1, :2 * n], pr["F0"] * RC.pitch_factor(SHIFTS[b]))
        eN = rel_err(rag["N"][b:b + 1, :2 * n], pr["N"])
        print(f"row {b} ({n} frames): F0 {eF:.2e} N {eN:.2e}")
        assert eF < 1e-4 and eN < 3e-2


def test_neutral_controls_are_the_call_without_them(eng, tiny):
    S, dev = tiny, eng.device
    h, codes = _inputs(S)
    prompt, eps = _sampler_inputs(S)

    def run(skw, pkw):
        n0 = eng.launches
        c = eng.sample_style(_h_act(eng, h), prompt.to(dev), eps.to(dev), STEPS, **skw).cpu().clone()
        pro = eng.predict_prosody(_h_act(eng, h), codes.to(dev), **pkw)
        out = _host(S, pro, False)
        out.update(codes=c, dsum=pro["dsum"].cpu().clone(), launches=eng.launches - n0)
        return out

    base = run(dict(cfg_scale=5.0), {})
    cases = [(dict(controls=rc), dict(controls=rc)) for rc in (
        eng.row_controls(B, cfg_scale=5.0),  # a scalar guidance scale is the scalar path
        eng.row_controls(B, cfg_scale=5.0, speed=1.0, pitch_shift=0.0),
        eng.row_controls(B, cfg_scale=5.0, speed=[1.0] * B, pitch_shift=[0.0] * B))]
    rc = eng.row_controls(B)  # nothing given: the cfg_scale argument applies
    cases.append((dict(cfg_scale=5.0, controls=rc), dict(controls=rc)))
    for skw, pkw in cases:
        got = run(skw, pkw)
        assert got["launches"] == base["launches"]
        for k in ("codes", "dur", "dsum", "idx", "en", "asr", "F0", "N"):
            assert torch.equal(got[k], base[k]), k
    assert eng.check_status() == 0


def test_mixed_rates_need_ragged_frames(eng, tiny):
    h, codes = _inputs(tiny)
    with pytest.raises(AssertionError, match="share its total frame count"):
        eng.predict_prosody(_h_act(eng, h), codes.to(eng.device), controls=eng.row_controls(B, speed=RATES))
    with pytest.raises(ValueError):
        eng.predict_prosody(_h_act(eng, h), codes.to(eng.device), controls=eng.row_controls(B + 1, speed=1.5))
    eng.check_status()


def test_captured_graph_replays_with_new_controls(gpu_device, eng, tiny, tiny_params):
    """captured once at n_frames = 96 (no host sync); set() between replays changes guidance, rate and pitch"""
    from stzs.engine import StyleTTSZS
    S = tiny
    e2 = StyleTTSZS(S, tiny_params, device=gpu_device)  # (its own buffer cache: a capture pins its shapes)
    h, codes = _inputs(S)
    prompt, eps = _sampler_inputs(S)
    A = dict(cfg_scale=SCALES, speed=RATES, pitch_shift=SHIFTS)
    Bc = dict(cfg_scale=[2.0, 0.0, 1.0, 3.0], speed=[2.0, 1.0, 0.5, 1.25], pitch_shift=[3.0, -12.0, 0.0, -1.0])

    def runner(e, rc):
        hd, pd, ed, cd = _h_act(e, h), prompt.to(gpu_device), eps.to(gpu_device), codes.to(gpu_device)

        def run():
            c = e.sample_style(hd, pd, ed, STEPS, controls=rc)
            pro = e.predict_prosody(hd, cd, n_frames=96, ragged_frames=True, controls=rc)
            return c, pro["dur"], pro["idx"], pro["en"].t, pro["F0"], pro["N"], pro["frame_lens"]
        return run

    eager = {}
    for name, kw in (("A", A), ("B", Bc)):
        eager[name] = [t.cpu().clone() for t in runner(eng, eng.row_controls(B, **kw))()]
    assert eng.check_status() == 0
    assert eager["A"][6].tolist() == FRAMES and eager["B"][6].tolist() == [24, 48, 96, 36]
    rc = e2.row_controls(B, **A)
    graph, outs = e2.capture(runner(e2, rc))
    for name, kw in (("A", None), ("B", Bc)):
        if kw is not None:
            rc.set(**kw)
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert graph.check() == 0
        for k, (a, b) in enumerate(zip(outs, eager[name])):
            assert torch.equal(a.cpu(), b), (name, k)
    with pytest.raises(ValueError):
        rc.set(cfg_scale=[1.0] * B)  # the CFG form would switch off: the graph holds the 2B-row launches
    with pytest.raises(ValueError):
        e2.row_controls(B, speed=RATES).set(pitch_shift=SHIFTS)  # absent -> present


def test_synth_with_mixed_controls_matches_solo_synth(gpu_device, tiny):
    """the ragged decoder's spec (tests/test_gpu_ragged_decoder_stages.py): every row's waveform is its solo synth()
    with its own controls up to 600 frame_lens[b], exact zeros from there"""
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    S = tiny.replace(dec_out=128, gen_ch=(256, 128))
    e = StyleTTSZS(S, init_params(S, seed=2), device=gpu_device)
    e._check_ragged_decoder()
    g = torch.Generator().manual_seed(31)
    tok = torch.randint(1, S.n_symbols, (B, T), generator=g)
    N = S.sr // 2
    ref = torch.randn(B, N, generator=g) * 0.1
    eps = torch.randn(B, S.L_s, S.code_dim, generator=g)
    rc = e.row_controls(B, cfg_scale=SCALES, speed=RATES, pitch_shift=SHIFTS)
    wav, fl = e.synth(tok, ref, steps=STEPS, noise=eps, seeds=[3, 4, 5, 6], ragged_frames=True, controls=rc)
    wav, fl = wav.cpu().clone(), fl.cpu().tolist()
    print("frame counts", fl)
    assert wav.shape == (B, S.frame40 * max(fl)) and len(set(fl)) > 1
    for b in range(B):
        one = e.synth(tok[b:b + 1], ref[b:b + 1], steps=STEPS, cfg_scale=SCALES[b], noise=eps[b:b + 1], seeds=[3 + b],
                      controls=e.row_controls(1, speed=RATES[b], pitch_shift=SHIFTS[b]))["wav"].cpu()
        assert one.shape == (1, S.frame40 * fl[b]), (one.shape, fl[b])
        _near(f"row {b} waveform", wav[b, :one.shape[1]], one[0])
        assert bool((wav[b, one.shape[1]:] == 0).all())
    # synth_stream takes the same controls: its chunks are the waveform above
    parts = [c.clone() for _, c in e.synth_stream(tok, ref, steps=STEPS, noise=eps, seeds=[3, 4, 5, 6], chunk_s=0.5,
                                                   ragged_frames=True, controls=rc)]
    assert len(parts) > 1 and e.frame_lens.cpu().tolist() == fl
    assert torch.equal(torch.cat(parts, 1).cpu(), wav)
    # the scalar argument still applies when the controls carry no guidance scale
    a = e.synth(tok[:1], ref[:1], steps=STEPS, cfg_scale=2.5, noise=eps[:1], seeds=[3],
                controls=e.row_controls(1, speed=1.7))["wav"].cpu().clone()
    b_ = e.synth(tok[:1], ref[:1], steps=STEPS, noise=eps[:1], seeds=[3],
                 controls=e.row_controls(1, cfg_scale=2.5, speed=1.7))["wav"].cpu()
    assert torch.equal(a, b_)
