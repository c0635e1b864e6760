"""BucketScheduler(ragged_decoder=True) (stzs/scheduler.py): the request mix of
tests/test_gpu_ragged_frames_scheduler.py (7 requests, max_batch 4) on the smallest spec whose generator takes the
length-aware conv forms, with all four ragged flags.  Every waveform must be bit-identical to the same request
synthesized alone; phase 2 runs as many decoder passes as prosody batches -- two."""
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


def test_ragged_decoder_scheduler_matches_single_requests(gpu_device, tiny):
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.scheduler import BucketScheduler
    S = tiny.replace(dec_out=128, gen_ch=(256, 128))
    eng = StyleTTSZS(S, init_params(S, seed=2), device=gpu_device)
    reqs = _reqs(S)
    wavs = [eng.synth(r.tokens[None], r.ref_wav[None], steps=STEPS, cfg_scale=CFG, noise=r.noise[None],
                      durations=r.durations[None] if r.durations is not None else None,
                      seeds=[r.seed])["wav"][0].clone() for r in reqs]
    sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG, ragged_text=True, ragged_ref=True,
                          ragged_frames=True, ragged_decoder=True)
    outs = sch.synth(reqs)
    st = sch.stats
    print("ragged-decoder scheduler", st)
    frames = [w.shape[0] // S.frame40 for w in wavs]
    assert st["decoder_batches"] == 2 and st["prosody_batches"] == 2 and st["phase2_batches"] == 2
    chunks, _ = sch.phase2_groups(frames)
    pad = sum(max(frames[i] for i in ch) * len(ch) - sum(frames[i] for i in ch) for ch in chunks)
    assert abs(st["decoder_pad_share"] - pad / sum(max(frames[i] for i in ch) * len(ch) for ch in chunks)) < 1e-12
    for r, w, one, n in zip(reqs, outs, wavs, frames):
        assert w.shape == one.shape
        assert torch.equal(w, one), f"request of {n} frames: waveform differs from its solo synth()"
