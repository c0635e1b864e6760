"""BucketScheduler(ragged_frames=True) (stzs/scheduler.py): the request mix of
tests/test_gpu_ragged_ref_scheduler.py with ragged_frames alone and with all three ragged flags.  Every waveform must
equal the same request synthesized alone (that file's bound: bit-identical expected, asserted max-abs <= 1e-6 of
max|ref|); prosody runs in as many batches as phase2_groups says -- one per max_batch requests, fewer than the
decoder's frame buckets."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, CFG = 2, 5.0


def _reqs(S):
    from stzs.scheduler import Request
    g = torch.Generator().manual_seed(21)
    short = S.mel_nfft // 2 + 1
    reqs = []
    for k, (T, nref, forced) in enumerate([(8, S.sr, None), (12, 7 * S.sr // 10 + 1, None), (12, S.sr, None),
                                           (8, S.sr + S.sr // 2, None), (10, short, [4] * 10), (8, S.sr, [5] * 8),
                                           (6, short, None)]):
        reqs.append(Request(tokens=torch.randint(1, S.n_symbols, (T,), generator=g),
                            ref_wav=torch.randn(nref, generator=g) * 0.1,
                            noise=torch.randn(S.L_s, S.code_dim, generator=g), seed=100 + k,
                            durations=torch.tensor(forced, dtype=torch.int32) if forced else None))
    return reqs


@pytest.fixture(scope="module")
def solo(gpu_device, tiny, tiny_params):
    """the engine and every request's own synth(), computed once"""
    from stzs.engine import StyleTTSZS
    eng = StyleTTSZS(tiny, tiny_params, device=gpu_device)
    reqs = _reqs(tiny)
    wavs = [eng.synth(r.tokens[None], r.ref_wav[None], steps=STEPS, cfg_scale=CFG, noise=r.noise[None],
                      durations=r.durations[None] if r.durations is not None else None,
                      seeds=[r.seed])["wav"][0].clone() for r in reqs]
    return eng, reqs, wavs


@pytest.mark.parametrize("others", [False, True], ids=["frames", "frames+text+ref"])
def test_ragged_frames_scheduler_matches_single_requests(solo, others):
    from stzs.scheduler import BucketScheduler
    eng, reqs, wavs = solo
    sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG, ragged_text=others, ragged_ref=others,
                          ragged_frames=True)
    outs = sch.synth(reqs)
    st = sch.stats
    print("ragged-frames scheduler", st)
    frames = [w.shape[0] // eng.spec.frame40 for w in wavs]
    pros, dec = sch.phase2_groups(frames)
    assert st["prosody_batches"] == len(pros) == 2  # 7 requests in chunks of 4, whatever their frame counts
    assert st["phase2_batches"] == len(dec) and st["prosody_batches"] < st["phase2_batches"]
    assert st["frame_buckets"] == sorted(set(frames)) and 0.0 < st["frame_pad_share"] < 1.0
    for r, w, one in zip(reqs, outs, wavs):
        assert w.shape == one.shape
        err = ((w - one).abs().max() / one.abs().max()).item()
        print("len", w.shape[0], "equal" if torch.equal(w, one) else f"max-rel {err:.2e}")
        assert err <= 1e-6
