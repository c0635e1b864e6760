"""BucketScheduler with per-request controls (stzs/scheduler.py): 7 requests, max_batch 4, some at the
defaults and some with their own guidance scale, speaking rate and pitch shift.  On SPEC_TINY with the flags off and
with ragged_text + ragged_ref + ragged_frames, on the ragged decoder's spec with ragged_decoder too.  Every waveform
must equal the same request synthesized alone with its controls (max-abs <= 1e-6 of max|ref|; bit-identical is
expected and which one held is printed).  With all-default requests no controls are built: the waveforms are the solo
ones and the statistics are those of the groupings."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, CFG = 2, 5.0
#            cfg_scale, speed, pitch_shift (None / 1 / 0: the defaults)
CONTROLS = [(None, 1.0, 0.0), (1.0, 1.0, 0.0), (2.5, 0.5, 12.0), (None, 1.7, 0.0), (0.0, 1.0, -7.0), (None, 4.0, 3.5),
            (None, 1.0, 0.0)]


def _reqs(S, controls=True):
    from stzs.scheduler import Request
    g = torch.Generator().manual_seed(21)
    short = S.mel_nfft // 2 + 1
    reqs = []
    for k, (T, nref, forced) in enumerate([(8, S.sr, None), (8, S.sr, None), (12, S.sr, None), (12, S.sr, None),
                                           (8, S.sr, None), (10, short, [4] * 10), (8, S.sr, None)]):
        r = Request(tokens=torch.randint(1, S.n_symbols, (T,), generator=g),
                    ref_wav=torch.randn(nref, generator=g) * 0.1,
                    noise=torch.randn(S.L_s, S.code_dim, generator=g), seed=100 + k,
                    durations=torch.tensor(forced, dtype=torch.int32) if forced else None)
        if controls:
            r.cfg_scale, r.speed, r.pitch_shift = CONTROLS[k]
        reqs.append(r)
    return reqs


def _solo(eng, r):
    rc = eng.row_controls(1, speed=r.speed, pitch_shift=r.pitch_shift)
    return eng.synth(r.tokens[None], r.ref_wav[None], steps=STEPS, cfg_scale=CFG if r.cfg_scale is None else r.cfg_scale,
                     noise=r.noise[None], durations=r.durations[None] if r.durations is not None else None,
                     seeds=[r.seed], controls=rc)["wav"][0].clone()


def _check(outs, wavs):
    bits = 0
    for k, (w, one) in enumerate(zip(outs, wavs)):
        assert w.shape == one.shape, (k, w.shape, one.shape)
        err = ((w - one).abs().max() / one.abs().max()).item()
        bits += int(torch.equal(w, one))
        assert err <= 1e-6, f"request {k} {CONTROLS[k]}: waveform differs from its solo synth(): {err:.2e}"
    print(f"{bits} of {len(outs)} waveforms bit-identical to the solo synth()")


@pytest.fixture(scope="module")
def eng(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    return StyleTTSZS(tiny, tiny_params, device=gpu_device)


@pytest.fixture(scope="module")
def solos(eng, tiny):
    return [_solo(eng, r) for r in _reqs(tiny)]


@pytest.mark.parametrize("flags", [dict(), dict(ragged_text=True, ragged_ref=True, ragged_frames=True)],
                         ids=["uniform", "ragged"])
def test_mixed_controls_match_single_requests(eng, tiny, solos, flags):
    from stzs.scheduler import BucketScheduler
    S = tiny
    reqs = _reqs(S)
    sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG, **flags)
    outs = sch.synth(reqs)
    print("controls scheduler", flags, sch.stats)
    assert len({w.shape[0] for w in solos}) > 2  # the rates gave the requests different frame counts
    _check(outs, solos)
    assert sch.stats["control_batches"] >= 2
    assert sch.stats["phase1_batches"] == len(sch.phase1_groups(reqs))  # no group was split by a control


def test_mixed_controls_with_the_ragged_decoder(gpu_device, tiny):
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.scheduler import BucketScheduler
    S = tiny.replace(dec_out=128, gen_ch=(256, 128))
    e = StyleTTSZS(S, init_params(S, seed=2), device=gpu_device)
    reqs = _reqs(S)
    wavs = [_solo(e, r) for r in reqs]
    sch = BucketScheduler(e, max_batch=4, steps=STEPS, cfg_scale=CFG, ragged_text=True, ragged_ref=True,
                          ragged_frames=True, ragged_decoder=True)
    outs = sch.synth(reqs)
    print("controls scheduler, ragged decoder", sch.stats)
    _check(outs, wavs)
    # both flags on: phase 1 is keyed by (forced,) alone, phase 2 runs the 7 requests as 2 ragged chunks
    assert sch.stats["phase1_batches"] == len(sch.phase1_groups(reqs)) == 3 and sch.stats["phase2_batches"] == 2
    assert sch.stats["control_batches"] >= 2


def test_default_requests_build_no_controls(eng, tiny, monkeypatch):
    from stzs.scheduler import BucketScheduler
    S = tiny
    reqs = _reqs(S, controls=False)
    wavs = [eng.synth(r.tokens[None], r.ref_wav[None], steps=STEPS, cfg_scale=CFG, noise=r.noise[None],
                      durations=r.durations[None] if r.durations is not None else None,
                      seeds=[r.seed])["wav"][0].clone() for r in reqs]
    made = []
    real = eng.row_controls
    monkeypatch.setattr(eng, "row_controls", lambda *a, **kw: made.append(a) or real(*a, **kw))
    for flags in (dict(), dict(ragged_text=True, ragged_ref=True, ragged_frames=True)):
        sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG, **flags)
        outs = sch.synth(reqs)
        st = sch.stats
        assert not made and st["control_batches"] == 0
        for k, (w, one) in enumerate(zip(outs, wavs)):
            assert torch.equal(w, one), (flags, k)
        frames = [w.shape[0] // S.frame40 for w in wavs]
        pros, dec = sch.phase2_groups(frames)
        assert st["requests"] == 7 and st["phase1_batches"] == len(sch.phase1_groups(reqs))
        assert st["phase2_batches"] == st["decoder_batches"] == len(dec) and st["prosody_batches"] == len(pros)
        assert st["frame_buckets"] == sorted(set(frames))
        assert set(st) == {"requests", "phase1_batches", "phase2_batches", "control_batches", "frame_buckets",
                           "phase1_ms", "ref_pad_share", "prosody_batches", "frame_pad_share", "decoder_batches",
                           "decoder_pad_share"}
