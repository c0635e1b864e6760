"""BucketScheduler(ragged_ref=True) (stzs/scheduler.py): the request mix of tests/test_gpu_scheduler.py
with its references cut to four different lengths -- 1 s, 1.5 s, 0.7 s + 1 sample and the shortest legal clip
(mel_nfft / 2 + 1 samples) -- with ragged_ref alone and with ragged_text as well.  Every waveform must equal the same
request synthesized alone (that file's bound: bit-identical expected, asserted max-abs <= 1e-6 of max|ref|), in as
many phase-1 batches as phase1_groups says."""
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


@pytest.mark.parametrize("ragged_text,n_want", [(False, 5), (True, 3)], ids=["ref", "ref+text"])
def test_ragged_ref_scheduler_matches_single_requests(solo, ragged_text, n_want):
    from stzs.scheduler import BucketScheduler
    eng, reqs, wavs = solo
    sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG, ragged_text=ragged_text, ragged_ref=True)
    outs = sch.synth(reqs)
    print("ragged-ref scheduler", sch.stats)
    n_groups = len(sch.phase1_groups(reqs))
    n_plain = len(BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG).phase1_groups(reqs))
    # ragged_ref alone: by (token count, forced) -- 8: [0, 3], 12: [1, 2], 10 forced, 8 forced, 6; both: unforced
    # [0, 1, 2, 3] + [6], forced [4, 5]
    assert sch.stats["phase1_batches"] == n_groups == n_want and n_groups < n_plain == 7
    assert 0.0 < sch.stats["ref_pad_share"] < 1.0
    for r, w, one in zip(reqs, outs, wavs):
        assert w.shape == one.shape
        err = ((w - one).abs().max() / one.abs().max()).item()
        print("len", w.shape[0], "ref", r.ref_wav.shape[0], "equal" if torch.equal(w, one) else f"max-rel {err:.2e}")
        assert err <= 1e-6
