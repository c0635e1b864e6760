"""BucketScheduler with all four ragged flags on the PRECISE engine: the 7-request mix and max_batch 4
of tests/test_gpu_ragged_decoder_scheduler.py on StyleTTSZS(precise=True).  Every waveform must be bit-identical to the
same request synthesized alone on that engine; phase 2 runs fewer prosody and decoder batches than there are requests."""
import pytest
import torch

from test_gpu_ragged_decoder_scheduler import CFG, STEPS, _reqs

pytestmark = pytest.mark.gpu


def test_ragged_precise_scheduler_matches_single_requests(gpu_device, tiny):
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.scheduler import BucketScheduler
    S = tiny.replace(dec_out=128, gen_ch=(256, 128))
    eng = StyleTTSZS(S, init_params(S, seed=2), device=gpu_device, precise=True)
    reqs = _reqs(S)
    wavs = [eng.synth(r.tokens[None], r.ref_wav[None], steps=STEPS, cfg_scale=CFG, noise=r.noise[None],
                      durations=r.durations[None] if r.durations is not None else None,
                      seeds=[r.seed])["wav"][0].clone() for r in reqs]
    sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG, ragged_text=True, ragged_ref=True,
                          ragged_frames=True, ragged_decoder=True)
    outs = sch.synth(reqs)
    st = sch.stats
    print("ragged precise scheduler", st)
    frames = [w.shape[0] // S.frame40 for w in wavs]
    assert st["prosody_batches"] < len(reqs) and st["decoder_batches"] < len(reqs)
    assert st["decoder_batches"] == 2 and st["prosody_batches"] == 2  # (7 requests in chunks of max_batch 4)
    for w, one, n in zip(outs, wavs, frames):
        assert w.shape == one.shape
        assert torch.equal(w, one), f"request of {n} frames: waveform differs from its solo synth()"
    assert eng.check_status() == 0
