"""Sample rates through the engine, the scheduler and the torch operator, SPEC_TINY, default engine.
Every check is bit equality against the composition it stands for -- the same launches made by hand -- but for the
resampled reference, which is also held to the kernel's derived bound against the float64 reference.  The ragged and
streaming cases run on the smallest spec that passes _check_ragged_decoder (dec_out 128, gen_ch (256, 128), as
tests/test_gpu_ragged_decoder_stages.py)."""
import numpy as np
import pytest
import torch

import refops_resample as R

pytestmark = pytest.mark.gpu

B, T = 4, 8
STEPS, CFG = 2, 5.0
N16 = 8000
LENS16 = [8000, 5601, 8000, 700]      # at 16 kHz; 700 -> 1050 samples at 24 kHz, just above mel_nfft / 2 + 1
FRAMES = [7, 1, 3, 6]


def _inputs(S, frames=None):
    g = torch.Generator().manual_seed(47)
    tok = torch.randint(1, S.n_symbols, (B, T), generator=g)
    r16 = torch.randn(B, N16, generator=g) * 0.1
    eps = torch.randn(B, S.L_s, S.code_dim, generator=g)
    dur = torch.zeros(B, T, dtype=torch.int32)
    for b in range(B):
        n = 8 if frames is None else frames[b]
        dur[b] = torch.tensor([n // T + (1 if t < n % T else 0) for t in range(T)], dtype=torch.int32)
    return tok, r16, eps, dur


@pytest.fixture(scope="module")
def eng(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    return StyleTTSZS(tiny, tiny_params, device=gpu_device)


@pytest.fixture(scope="module")
def rag(gpu_device, tiny):
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    S = tiny.replace(dec_out=128, gen_ch=(256, 128))
    e = StyleTTSZS(S, init_params(S, seed=2), device=gpu_device)
    e._check_ragged_decoder()
    return e


def _keep(out):
    return {k: out[k].clone() for k in ("prompt_idx", "codes", "wav")}


# ---- the reference side ----------------------------------------------------------------------------------------------

def test_ref_sr_is_the_composition_of_resample_and_synth(eng, tiny):
    from stzs.resample import design, out_len
    S = tiny
    tok, r16, eps, dur = _inputs(S)
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[1, 2, 3, 4])
    L, M, W, K, o, h = design(16000, S.sr)
    mapped = [out_len(n, L, M) for n in LENS16]
    n0 = eng.launches
    got = _keep(eng.synth(tok, r16, ref_sr=16000, ref_lens=LENS16, **kw))
    n_with = eng.launches - n0
    r24, ol = eng.resample(r16, 16000, S.sr, LENS16)
    assert ol.cpu().tolist() == mapped and r24.shape == (B, out_len(N16, L, M))
    n0 = eng.launches
    want = _keep(eng.synth(tok, r24, ref_lens=mapped, **kw))
    assert n_with == eng.launches - n0 + 1  # one launch more than the 24 kHz call
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # device lengths: mapped by the kernel, the same bits
    dl = torch.tensor(LENS16, dtype=torch.int32, device=eng.device)
    dev = _keep(eng.synth(tok, r16.to(eng.device), ref_sr=16000, ref_lens=dl, **kw))
    for k in want:
        assert torch.equal(dev[k], want[k]), k
    # ref_sr at the model's own rate: the call as it was
    same = _keep(eng.synth(tok, r24, ref_sr=S.sr, ref_lens=mapped, **kw))
    assert torch.equal(same["wav"], want["wav"])
    # the resampled reference against float64 with the kernel's bound; past a row's end exact zeros
    worst = 0.0
    r24h = r24.cpu()
    for b, n in enumerate(LENS16):
        y64, sabs = R.resample_ref(r16[b].numpy(), h, o, L, M, K, n=n)
        err = np.abs(r24h[b, :mapped[b]].numpy().astype(np.float64) - y64)
        bound = (K + 1) * 2.0 ** -24 * sabs
        assert (err <= bound).all(), b
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert not r24h[b, mapped[b]:].any()
    print(f"16 -> 24 kHz reference: largest error / bound {worst:.3f}")
    # host lengths are checked at the model's rate: 600 samples at 16 kHz are 900, below mel_nfft / 2 + 1
    with pytest.raises(ValueError):
        eng.synth(tok, r16, ref_sr=16000, ref_lens=[8000, 8000, 8000, 600], **kw)
    with pytest.raises(ValueError):
        eng.synth(tok, r16, ref_sr=16000, ref_lens=[8001, 8000, 8000, 8000], **kw)


# ---- the output side -------------------------------------------------------------------------------------------------

def test_out_sr_and_out_dtype(eng, tiny):
    S = tiny
    tok, r16, eps, dur = _inputs(S)
    ref = torch.randn(B, S.sr // 2, generator=torch.Generator().manual_seed(3)) * 0.1
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[1, 2, 3, 4])
    n0 = eng.launches
    base = eng.synth(tok, ref, **kw)
    n_base = eng.launches - n0
    assert "sr" not in base
    wav = base["wav"].clone()
    n0 = eng.launches
    o48 = eng.synth(tok, ref, out_sr=48000, **kw)
    assert eng.launches - n0 == n_base + 1
    assert o48["sr"] == 48000 and o48["wav"].dtype == torch.float32 and o48["wav"].shape == (B, 2 * wav.shape[1])
    assert torch.equal(o48["wav"], eng.resample(wav, S.sr, 48000)[0])
    o16 = eng.synth(tok, ref, out_sr=16000, out_dtype=torch.int16, **kw)
    assert o16["sr"] == 16000 and o16["wav"].dtype == torch.int16
    assert torch.equal(o16["wav"], eng.resample(wav, S.sr, 16000, dtype=torch.int16)[0])
    pcm = eng.synth(tok, ref, out_dtype=torch.int16, **kw)  # the identity filter: fp32 -> PCM16 at 24 kHz
    assert pcm["sr"] == S.sr
    assert torch.equal(pcm["wav"], torch.clamp(torch.round(32768.0 * wav), -32768, 32767).to(torch.int16))
    same = eng.synth(tok, ref, out_sr=S.sr, **kw)
    assert same["sr"] == S.sr and torch.equal(same["wav"], wav)
    with pytest.raises(ValueError):
        eng.synth(tok, ref, out_sr=24001, **kw)
    with pytest.raises(ValueError):
        eng.synth(tok, ref, out_dtype=torch.float16, **kw)


def test_out_sr_with_ragged_frames(rag):
    from stzs.resample import out_len
    S = rag.spec
    tok, r16, eps, dur = _inputs(S, FRAMES)
    ref = torch.randn(B, S.sr // 2, generator=torch.Generator().manual_seed(3)) * 0.1
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[1, 2, 3, 4], ragged_frames=True)
    wav24, fl = rag.synth(tok, ref, **kw)
    wav24 = wav24.clone()
    assert fl.cpu().tolist() == FRAMES
    for sr, dt, (L, M) in ((16000, torch.float32, (2, 3)), (44100, torch.int16, (147, 80))):
        wav, fl2 = rag.synth(tok, ref, out_sr=sr, out_dtype=dt, **kw)
        assert fl2.cpu().tolist() == FRAMES and wav.shape == (B, out_len(wav24.shape[1], L, M)) and wav.dtype == dt
        for b, n in enumerate(FRAMES):
            solo = rag.resample(wav24[b:b + 1, :S.frame40 * n], S.sr, sr, dtype=dt)[0]
            nb = out_len(S.frame40 * n, L, M)
            assert solo.shape == (1, nb)
            assert torch.equal(wav[b, :nb], solo[0]), (sr, b)
            assert not wav[b, nb:].any(), (sr, b)


# ---- streaming -------------------------------------------------------------------------------------------------------

def _cat(gen):
    parts, end = [], 0
    for n0, w in gen:
        assert n0 == end, (n0, end)  # contiguous
        assert w.shape[1] > 0
        end += w.shape[1]
        parts.append(w.clone())
    return torch.cat(parts, 1)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("halo", [None, 1], ids=["exact", "chunked"])
def test_synth_stream_out_sr(rag, halo, ragged):
    S = rag.spec
    tok, r16, eps, dur = _inputs(S, FRAMES if ragged else None)
    ref = torch.randn(B, S.sr // 2, generator=torch.Generator().manual_seed(3)) * 0.1
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[1, 2, 3, 4], ragged_frames=ragged,
              chunk_s=2 * S.frame40 / S.sr, chunked_halo=halo)
    plain = _cat(rag.synth_stream(tok, ref, **kw))
    fl = rag.frame_lens.clone() if ragged else None
    for sr, dt in ((48000, torch.float32), (16000, torch.int16)):
        got = _cat(rag.synth_stream(tok, ref, out_sr=sr, out_dtype=dt, **kw))
        want = rag.resample(plain, S.sr, sr, lens=fl, lens_mul=S.frame40 if ragged else 1, dtype=dt)[0]
        assert got.dtype == dt and got.shape == want.shape
        assert torch.equal(got, want), (sr, halo, ragged)
    # a reference at another rate in front of a stream: the composition again
    r24, _ = rag.resample(r16, 16000, S.sr)
    a = _cat(rag.synth_stream(tok, r16, ref_sr=16000, **kw))
    assert torch.equal(a, _cat(rag.synth_stream(tok, r24, **kw)))


# ---- graph capture ---------------------------------------------------------------------------------------------------

def test_captured_synth_with_both_rates(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    S = tiny
    e = StyleTTSZS(S, tiny_params, device=gpu_device)  # (its own buffer cache: a capture pins its shapes)
    tok, r16, eps, dur = _inputs(S)
    tok_d, r16_d, eps_d, dur_d = (t.to(gpu_device) for t in (tok.to(torch.int32), r16, eps, dur))
    dl = torch.tensor(LENS16, dtype=torch.int32, device=gpu_device)
    nf = int(dur[0].sum())

    def fn():
        o = e.synth(tok_d, r16_d, steps=STEPS, cfg_scale=CFG, noise=eps_d, durations=dur_d, seeds=[1, 2, 3, 4],
                    n_frames=nf, ref_sr=16000, ref_lens=dl, out_sr=44100, out_dtype=torch.int16, check=False)
        return o["wav"], o["prompt_idx"], o["codes"]
    eager = [t.clone() for t in fn()]
    assert e.check_status() == 0
    graph, outs = e.capture(fn)
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert graph.check() == 0 and e.check_status() == 0
    for k, (a, b) in enumerate(zip(outs, eager)):
        assert torch.equal(a, b), k
    assert eager[0].dtype == torch.int16 and eager[0].any()


# ---- scheduler -------------------------------------------------------------------------------------------------------

RATES = [(None, None), (16000, None), (44100, 8000), (None, 48000), (16000, 48000), (44100, None), (None, 8000)]


def _reqs(S, rates=True):
    from stzs.scheduler import Request
    g = torch.Generator().manual_seed(21)
    reqs = []
    for k, (T_, secs) in enumerate([(8, 0.5), (8, 0.5), (12, 0.4), (12, 0.5), (8, 0.3), (10, 0.5), (8, 0.5)]):
        ref_sr, out_sr = RATES[k] if rates else (None, None)
        n = int(secs * (ref_sr or S.sr))
        reqs.append(Request(tokens=torch.randint(1, S.n_symbols, (T_,), generator=g),
                            ref_wav=torch.randn(n, generator=g) * 0.1,
                            noise=torch.randn(S.L_s, S.code_dim, generator=g), seed=100 + k,
                            ref_sr=ref_sr, out_sr=out_sr))
    return reqs


def _solo(eng, r):
    return eng.synth(r.tokens[None], r.ref_wav[None], steps=STEPS, cfg_scale=CFG, noise=r.noise[None], seeds=[r.seed],
                     ref_sr=r.ref_sr, out_sr=r.out_sr)["wav"][0].clone()


def test_scheduler_with_mixed_rates(eng, tiny):
    from stzs.scheduler import BucketScheduler
    S = tiny
    reqs = _reqs(S)
    solos = [_solo(eng, r) for r in reqs]
    sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG, ragged_text=True, ragged_ref=True)
    outs = sch.synth(reqs)
    print("resample scheduler", sch.stats)
    for k, (w, one) in enumerate(zip(outs, solos)):
        assert w.shape == one.shape and torch.equal(w, one), (k, RATES[k])
    assert sch.stats["resample_batches"] == 4  # 16 and 44.1 kHz in, 8 and 48 kHz out
    assert reqs[1].ref_sr == 16000 and reqs[1].ref_wav.shape[0] == 8000  # the caller's requests are left alone


def test_scheduler_at_the_defaults(eng, tiny, monkeypatch):
    from stzs.scheduler import BucketScheduler
    S = tiny
    reqs = _reqs(S, rates=False)
    solos = [_solo(eng, r) for r in reqs]
    made = []
    real = eng.resample
    monkeypatch.setattr(eng, "resample", lambda *a, **kw: made.append(a) or real(*a, **kw))
    sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG)
    outs = sch.synth(reqs)
    assert not made and sch.stats["resample_batches"] == 0
    assert set(sch.stats) == {"requests", "phase1_batches", "phase2_batches", "control_batches", "frame_buckets",
                              "phase1_ms", "ref_pad_share", "prosody_batches", "frame_pad_share", "decoder_batches",
                              "decoder_pad_share"}
    for k, (w, one) in enumerate(zip(outs, solos)):
        assert torch.equal(w, one), k


# ---- torch operator --------------------------------------------------------------------------------------------------

def test_torch_operator(gpu_device):
    from stzs import ops  # noqa: F401
    from stzs.resample import resampler
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(3, 3000, generator=g) * 0.4).to(gpu_device)
    lens = torch.tensor([3000, 17, 2999], dtype=torch.int32, device=gpu_device)
    for a, b in ((24000, 44100), (48000, 24000), (24000, 24000)):
        rs = resampler(gpu_device, a, b)
        for pcm in (False, True):
            y, n = torch.ops.stzs.resample(x, a, b, lens, pcm)
            yw, nw = rs(x, lens, dtype=torch.int16 if pcm else torch.float32)
            assert y.dtype == (torch.int16 if pcm else torch.float32)
            assert torch.equal(y, yw) and torch.equal(n, nw)
        y, n = torch.ops.stzs.resample(x, a, b)
        assert torch.equal(y, rs(x)[0]) and n.cpu().tolist() == [rs.out_len(3000)] * 3
    with pytest.raises(NotImplementedError):
        torch.ops.stzs.resample(x.cpu(), 24000, 48000)
    with pytest.raises(ValueError):
        torch.ops.stzs.resample(x, 24000, 24001)
