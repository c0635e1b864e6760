"""BucketScheduler with enrolled voices (stzs/scheduler.py) on SPEC_TINY: six requests over two
single-clip voices whose clips differ in length, different texts, some with controls and an output rate.  Every waveform
must EQUAL the one of the same request carrying its voice's clip as ref_wav through the same scheduler configuration;
voice requests batch together whatever their clips' lengths were; a blended request equals engine.synth of it alone; a
list without voices has the statistics it had before voices existed."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, CFG = 2, 5.0
CLIP_N = [3000, 4200]
#        tokens, voice, speed, pitch_shift, out_sr
ROWS = [(8, 0, 1.0, 0.0, None), (8, 1, 1.0, 0.0, None), (10, 0, 1.5, 0.0, None), (10, 1, 1.0, -5.0, 16000),
        (12, 1, 1.0, 0.0, None), (8, 0, 1.0, 0.0, 16000)]
STAT_KEYS = {"requests", "phase1_batches", "phase2_batches", "control_batches", "frame_buckets", "phase1_ms",
             "ref_pad_share", "prosody_batches", "frame_pad_share", "decoder_batches", "decoder_pad_share"}


@pytest.fixture(scope="module")
def eng(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    return StyleTTSZS(tiny, tiny_params, device=gpu_device)


@pytest.fixture(scope="module")
def clips():
    g = torch.Generator().manual_seed(31)
    return [torch.randn(n, generator=g) * 0.1 for n in CLIP_N]


@pytest.fixture(scope="module")
def voices(eng, clips):
    return [eng.enroll(c) for c in clips]


def _reqs(S, clips, voices):
    """the six requests, as voice requests (voices given) or carrying the voice's clip"""
    from stzs.scheduler import Request
    g = torch.Generator().manual_seed(32)
    out = []
    for k, (T, v, speed, pitch, osr) in enumerate(ROWS):
        tok = torch.randint(1, S.n_symbols, (T,), generator=g)
        eps = torch.randn(S.L_s, S.code_dim, generator=g)
        out.append(Request(tokens=tok, ref_wav=None if voices else clips[v], noise=eps, seed=50 + k, speed=speed,
                           pitch_shift=pitch, out_sr=osr, voice=voices[v] if voices else None))
    return out


@pytest.mark.parametrize("flags", [dict(), dict(ragged_text=True), dict(ragged_text=True, ragged_ref=True)],
                         ids=["uniform", "ragged_text", "ragged_text_ref"])
def test_voice_requests_equal_clip_requests(eng, tiny, clips, voices, flags):
    from stzs.scheduler import BucketScheduler
    S = tiny
    sch = BucketScheduler(eng, max_batch=8, steps=STEPS, cfg_scale=CFG, **flags)
    want = [w.clone() for w in sch.synth(_reqs(S, clips, None))]
    st_clip = dict(sch.stats)
    got = sch.synth(_reqs(S, clips, voices))
    st = sch.stats
    print("voice scheduler", flags, st, "| clips:", st_clip)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), (flags, k)
    assert "voice_batches" not in st_clip and st["voice_batches"] >= 1
    assert st["voice_batches"] == st["phase1_batches"] == len(sch.phase1_groups(_reqs(S, clips, voices)))
    assert st["ref_pad_share"] == 0.0
    if not flags.get("ragged_ref"):  # the clips' lengths split the clip list's phase 1; voices have none
        assert st["phase1_batches"] < st_clip["phase1_batches"]
    if flags.get("ragged_text"):
        assert st["phase1_batches"] == 1  # six requests, whatever their texts and voices


def test_blended_request_equals_engine_synth(eng, tiny, clips, voices):
    from stzs.scheduler import BucketScheduler, Request
    from stzs.voice import VoiceBank
    S = tiny
    g = torch.Generator().manual_seed(33)
    tok = torch.randint(1, S.n_symbols, (9,), generator=g)
    eps = torch.randn(S.L_s, S.code_dim, generator=g)
    blend = Request(tokens=tok, ref_wav=None, noise=eps, seed=7, voice=[(voices[1], 1.0), (voices[0], 3.0)])
    pure = Request(tokens=tok, ref_wav=None, noise=eps, seed=8, voice=voices[0])
    sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG)
    got = [w.clone() for w in sch.synth([blend, pure])]
    assert sch.stats["voice_batches"] == 1 and sch.stats["phase1_batches"] == 1
    bank = VoiceBank(eng, 2)
    i0, i1 = bank.add(voices[0]), bank.add(voices[1])
    rows = eng.voice_rows(1, bank, [[i1, i0]], [[0.25, 0.75]])
    one = eng.synth(tok[None], None, steps=STEPS, cfg_scale=CFG, noise=eps[None], seeds=[7], voices=rows)["wav"][0]
    assert torch.equal(got[0], one)
    one = eng.synth(tok[None], clips[0][None], steps=STEPS, cfg_scale=CFG, noise=eps[None], seeds=[8])["wav"][0]
    assert torch.equal(got[1], one)
    with pytest.raises(ValueError):
        sch.synth([Request(tokens=tok, ref_wav=clips[0], noise=eps, voice=voices[0])])


def test_voice_free_list_has_the_statistics_from_before(eng, tiny, clips):
    from stzs.scheduler import BucketScheduler
    S = tiny
    reqs = _reqs(S, clips, None)
    for r in reqs:
        r.speed, r.pitch_shift, r.out_sr = 1.0, 0.0, None
    for flags in (dict(), dict(ragged_text=True, ragged_ref=True)):
        sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG, **flags)
        outs = sch.synth(reqs)
        st = sch.stats
        assert set(st) == STAT_KEYS and "voice_batches" not in st and st["voice_batches"] == 0
        frames = [w.shape[0] // S.frame40 for w in outs]
        pros, dec = sch.phase2_groups(frames)
        assert st["requests"] == 6 and st["phase1_batches"] == len(sch.phase1_groups(reqs))
        assert st["phase2_batches"] == st["decoder_batches"] == len(dec) and st["prosody_batches"] == len(pros)
        assert st["frame_buckets"] == sorted(set(frames)) and st["control_batches"] == 0
        for r, w in zip(reqs, outs):
            one = eng.synth(r.tokens[None], r.ref_wav[None], steps=STEPS, cfg_scale=CFG, noise=r.noise[None],
                            seeds=[r.seed])["wav"][0]
            assert torch.equal(w, one)
