"""Enrolled voices through the engine on SPEC_TINY: enrol, bank, per-row sources, synth / synth_stream /
captured graphs with voices=.  Every comparison is torch.equal: a voice enrolled from one clip IS that clip's prompt
features and codes, so synthesis from it is, bit for bit, synthesis from the clip; blends are held against the numpy
reference of tests/refops_voice.py and the oracle's product VQ."""
import numpy as np
import pytest
import torch

from refops_resample import PAIRS
from refops_voice import mix_ref, vq_ref

pytestmark = pytest.mark.gpu

T_TXT, N_REF = 8, 3000
STEPS, CFG = 2, 5.0
REF_LENS = [3000, 1025, 2200]  # (1025: the shortest clip the STFT's reflect padding takes)
FOREIGN = PAIRS[1][1]  # 16 kHz
FRONT_END = {"stft_frames", "fe.dft", "log_mel", "stft_logmel", "pe.conv0", "mask_rows", "pe.conv1", "pool_rows",
             "pe.proj", "code_quantize"}


@pytest.fixture(scope="module")
def engines(gpu_device, tiny, tiny_params):
    """default | latency | precise | fp8 engines, built on first use"""
    from stzs.engine import StyleTTSZS, latency_engine
    made = {}

    def get(name):
        if name not in made:
            if name == "default":
                made[name] = StyleTTSZS(tiny, tiny_params, device=gpu_device)
            elif name == "latency":
                made[name] = latency_engine(tiny, get("default").W, gpu_device)
            elif name == "precise":
                made[name] = StyleTTSZS(tiny, tiny_params, device=gpu_device, precise=True, precise_frontend=True)
            else:
                made[name] = StyleTTSZS(tiny, tiny_params, device=gpu_device, fp8_denoiser=True)
        return made[name]
    return get


def _inputs(S, B, seed=11):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, S.n_symbols, (B, T_TXT), generator=g)
    ref = torch.randn(B, N_REF, generator=g) * 0.1
    eps = torch.randn(B, S.L_s, S.code_dim, generator=g)
    dur = torch.tensor([[3, 2] * (T_TXT // 2)] * B, dtype=torch.int32)
    return tok, ref, eps, dur


def _traced(eng, fn):
    """fn() with every library launch of the engine recorded by name -> (result, names)"""
    names, call = [], eng._call

    def rec(f, arg, what, *a, **kw):
        names.append(what)
        return call(f, arg, what, *a, **kw)
    eng._call = rec
    try:
        return fn(), names
    finally:
        del eng._call


def _bank(eng, clips):
    from stzs.voice import VoiceBank
    bank = VoiceBank(eng, len(clips) + 1)
    voices = [eng.enroll(c) for c in clips]
    return bank, voices, [bank.add(v) for v in voices]


@pytest.mark.parametrize("name", ["default", "latency", "precise"])
def test_enrolled_clip_is_its_prompt(engines, tiny, name):
    eng = engines(name)
    S = tiny
    _, ref, _, _ = _inputs(S, 2)
    for b in range(2):
        v = eng.enroll(ref[b])
        z = eng.prompt_features(ref[b:b + 1].to(eng.device)).clone()
        q = eng.prompt_encode(ref[b:b + 1].to(eng.device)).clone()
        assert torch.equal(v.z, z[0]) and torch.equal(v.idx, eng.prompt_idx[0])
        assert v.clips == 1 and v.frontend == ("precise" if name == "precise" else "bf16")
        assert v.fingerprint == eng.voice_fingerprint()
        from oracle import stzs_ref as R
        assert torch.equal(q.cpu(), R.lookup_codes({"pe.vq": eng.W.t(eng.W.pe_vq).cpu()}, S, v.idx[None].cpu()))


@pytest.mark.parametrize("name,B", [("default", 1), ("default", 3), ("latency", 1), ("precise", 1), ("fp8", 1)])
def test_synth_from_voices_is_synth_from_clips(engines, tiny, name, B):
    eng = engines(name)
    S = tiny
    tok, ref, eps, dur = _inputs(S, B)
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=list(range(B)))
    bank, _, ids = _bank(eng, [ref[b] for b in range(B)])
    rows = eng.voice_rows(B, bank, ids)
    assert rows.gather
    keep = lambda o: {k: o[k].clone() for k in ("wav", "codes", "prompt_idx", "prompt")}
    n0 = eng.launches
    want, a = _traced(eng, lambda: keep(eng.synth(tok, ref, **kw)))
    n1 = eng.launches
    got, b = _traced(eng, lambda: keep(eng.synth(tok, None, voices=rows, **kw)))
    n2 = eng.launches
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert bool(torch.isfinite(got["wav"]).all())
    fe = [i for i, n in enumerate(a) if n in FRONT_END]
    assert fe and fe == list(range(fe[0], fe[-1] + 1)) and a[fe[-1]] == "code_quantize"
    assert b == a[:fe[0]] + ["voice_prompt"] + a[fe[-1] + 1:]  # one launch where the front end stood, nothing else
    assert (n1 - n0) - (n2 - n1) == len(fe) - 1
    if B == 3:  # the same voice in every row, and rows in another order
        rows.set([ids[2], ids[0], ids[2]])
        again = keep(eng.synth(tok, None, voices=rows, **kw))
        mixed = keep(eng.synth(tok, ref[[2, 0, 2]], **kw))
        for k in want:
            assert torch.equal(again[k], mixed[k]), k


def test_ragged_and_foreign_rate_enrolment(engines, tiny):
    eng = engines("default")
    g = torch.Generator().manual_seed(3)
    wav = torch.randn(3, N_REF, generator=g) * 0.1
    for b, n in enumerate(REF_LENS):
        wav[b, n:] = float("nan")  # (a read past a clip's end would poison the voice)
    for b, n in enumerate(REF_LENS):
        alone = eng.enroll(wav[b, :n])
        padded = eng.enroll(wav[b:b + 1], ref_lens=[n])
        assert torch.equal(padded.z, alone.z) and torch.equal(padded.idx, alone.idx), b
    # the ragged batch of all three, all the weight on one clip: that clip's voice (1 z + 0 z' + 0 z'')
    for b in range(3):
        one = eng.enroll(wav, ref_lens=REF_LENS, weights=[float(k == b) for k in range(3)])
        alone = eng.enroll(wav[b, :REF_LENS[b]])
        assert one.clips == 3 and torch.equal(one.idx, alone.idx)
        assert torch.equal(one.z + 0.0, alone.z + 0.0)  # (equal up to the sign of a zero: x + 0 z' loses a -0)
    # a clip at a foreign rate: padded + ref_lens equals the clip alone, both through ref_sr
    n16 = 1700
    w16 = torch.randn(1, 2000, generator=g) * 0.1
    w16[0, n16:] = float("nan")
    a = eng.enroll(w16[0, :n16], ref_sr=FOREIGN)
    b = eng.enroll(w16, ref_lens=[n16], ref_sr=FOREIGN)
    assert torch.equal(a.z, b.z) and torch.equal(a.idx, b.idx)
    r24, _ = eng.resample(w16[:, :n16].contiguous(), FOREIGN, tiny.sr)
    c = eng.enroll(r24[0].clone())
    assert torch.equal(a.z, c.z) and torch.equal(a.idx, c.idx)


def test_three_clip_voice_and_blends(engines, tiny):
    eng = engines("default")
    S = tiny
    dev = eng.device
    cb = eng.W.t(eng.W.pe_vq).cpu().numpy()
    g = torch.Generator().manual_seed(9)
    clips = torch.randn(3, N_REF, generator=g) * 0.1
    z3 = eng.prompt_features(clips.to(dev)).cpu().numpy().copy()
    third = np.float32(np.float64(1.0) / np.float64(3.0))
    voice = eng.enroll(clips)
    want = mix_ref(z3, [[0, 1, 2]], [[third] * 3], [3])
    assert voice.clips == 3 and voice.z.cpu().numpy().tobytes() == want[0].tobytes()
    wi, _ = vq_ref(cb, want)
    assert torch.equal(voice.idx.cpu(), wi[0])
    # weights: normalised in float64 on the host
    v2 = eng.enroll(clips, weights=[1, 2, 5])
    w = [np.float32(1 / 8), np.float32(2 / 8), np.float32(5 / 8)]
    assert v2.z.cpu().numpy().tobytes() == mix_ref(z3, [[0, 1, 2]], [w], [3])[0].tobytes()
    # a bank of the three single-clip voices: a (0.3, 0.7) blend, and a batch of one pure and one blended row
    bank, vs, ids = _bank(eng, [clips[k] for k in range(3)])
    zb = torch.stack([v.z for v in vs]).cpu().numpy()

    def prompt(rows):
        q = eng.voice_encode(rows).clone().cpu()
        return q, eng.prompt_idx.clone().cpu()
    blend = eng.voice_rows(1, bank, [[ids[0], ids[2]]], [[0.3, 0.7]])
    assert not blend.gather and blend.Kmax == 2
    q, idx = prompt(blend)
    zmix = mix_ref(zb, [[0, 2]], [[np.float32(0.3), np.float32(0.7)]], [2])
    wi, wq = vq_ref(cb, zmix)
    assert torch.equal(idx, wi) and torch.equal(q, wq)
    pure = eng.voice_rows(1, bank, [ids[1]])
    pq, pidx = prompt(pure)
    assert torch.equal(pidx[0], vs[1].idx.cpu())
    both = eng.voice_rows(2, bank, [[ids[1]], [ids[0], ids[2]]], [None, [0.3, 0.7]])
    assert not both.gather and both.cnt.tolist() == [1, 2]
    bq, bidx = prompt(both)
    assert torch.equal(bq[0], pq[0]) and torch.equal(bidx[0], pidx[0])
    assert torch.equal(bq[1], q[0]) and torch.equal(bidx[1], idx[0])
    # ... and through synth: each row of the batch is the row alone
    tok, _, eps, dur = _inputs(S, 2)
    kw = dict(steps=STEPS, cfg_scale=CFG, durations=dur[:1])
    two = eng.synth(tok, None, noise=eps, voices=both, steps=STEPS, cfg_scale=CFG, durations=dur, seeds=[4, 5])
    two = {k: two[k].clone() for k in ("wav", "codes")}
    for b, rows in enumerate((pure, blend)):
        one = eng.synth(tok[b:b + 1], None, noise=eps[b:b + 1], voices=rows, seeds=[4 + b], **kw)
        assert torch.equal(one["wav"][0], two["wav"][b]) and torch.equal(one["codes"][0], two["codes"][b]), b
    # the torch operator makes the engine's call
    from stzs import ops
    h = ops.register(eng)
    oi, oq = torch.ops.stzs.voice_prompt(h, bank.z, None, both.src, both.w, both.cnt)
    assert torch.equal(oi.cpu(), bidx) and torch.equal(oq.cpu(), bq)
    oi, oq = torch.ops.stzs.voice_prompt(h, bank.z, bank.idx, pure.src, pure.w, pure.cnt)
    assert torch.equal(oi.cpu(), pidx) and torch.equal(oq.cpu(), pq)
    # ... and the whole-pipeline operator with voices in place of the reference: both forms
    d = eng.device
    wav = torch.ops.stzs.synth_voices(h, tok.to(d), bank.z, None, both.src, both.w, both.cnt, eps.to(d), dur.to(d),
                                      STEPS, CFG, [4, 5])
    assert torch.equal(wav, two["wav"])
    wav = torch.ops.stzs.synth_voices(h, tok[:1].to(d), bank.z, bank.idx, pure.src, pure.w, pure.cnt, eps[:1].to(d),
                                      dur[:1].to(d), STEPS, CFG, [4])
    assert torch.equal(wav[0], two["wav"][0])


def test_stream_from_voices(engines, tiny):
    eng = engines("default")
    S = tiny
    B = 2
    tok, ref, eps, dur = _inputs(S, B)
    bank, _, ids = _bank(eng, [ref[0], ref[1]])
    rows = eng.voice_rows(B, bank, [[ids[0], ids[1]], [ids[1]]], [[1, 1], None])
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[0, 1])
    want = eng.synth(tok, None, voices=rows, **kw)["wav"].clone()
    chunks = [c.clone() for _, c in eng.synth_stream(tok, None, voices=rows, chunk_s=0.05, **kw)]
    assert len(chunks) > 1 and torch.equal(torch.cat(chunks, 1), want)


def test_conflicts_raise_before_any_launch(engines, tiny):
    eng = engines("default")
    S = tiny
    B = 2
    tok, ref, eps, dur = _inputs(S, B)
    bank, _, ids = _bank(eng, [ref[0], ref[1]])
    rows = eng.voice_rows(B, bank, ids)
    G = S.code_dim // S.vq_group
    n0 = eng.launches
    for r, kw in ((ref, {}), (None, dict(prompt_idx=torch.zeros(B, S.L_s, G, dtype=torch.int32))),
                  (None, dict(ref_lens=[N_REF] * B)), (None, dict(ref_sr=FOREIGN))):
        with pytest.raises(ValueError):
            eng.synth(tok, r, noise=eps, durations=dur, voices=rows, **kw)
        with pytest.raises(ValueError):
            next(eng.synth_stream(tok, r, noise=eps, durations=dur, voices=rows, **kw))
    assert eng.launches == n0


@pytest.mark.parametrize("form", ["gather", "mix"])
def test_captured_synth_replays_for_other_speakers(gpu_device, tiny, tiny_params, form):
    from stzs.engine import StyleTTSZS
    S = tiny
    eng = StyleTTSZS(S, tiny_params, device=gpu_device)  # (its own buffer cache: a capture pins its shapes)
    B = 2
    tok, ref, eps, dur = _inputs(S, B)
    clips = torch.cat([ref, torch.randn(2, N_REF, generator=torch.Generator().manual_seed(77)) * 0.1])
    bank, vs, ids = _bank(eng, [clips[k] for k in range(3)])
    v_new = eng.enroll(clips[3])
    if form == "gather":
        first, other = dict(ids=[0, 1]), dict(ids=[2, 0])
    else:
        first = dict(ids=[[0, 1], [1]], weights=[[0.3, 0.7], None])
        other = dict(ids=[[2], [1, 0]], weights=[None, [0.9, 0.1]])
    rows = eng.voice_rows(B, bank, **first)
    tok_d, eps_d, dur_d = tok.to(gpu_device, torch.int32), eps.to(gpu_device), dur.to(gpu_device)
    nf = int(dur[0].sum())

    def fn(r=rows):
        o = eng.synth(tok_d, None, steps=STEPS, cfg_scale=CFG, noise=eps_d, durations=dur_d, seeds=[0, 1], n_frames=nf,
                      voices=r, check=False)
        return o["wav"], o["prompt_idx"], o["codes"]

    def eager(**kw):
        e = [t.clone() for t in fn(eng.voice_rows(B, bank, **kw))]
        assert eng.check_status() == 0
        return e
    want0 = eager(**first)
    graph, outs = eng.capture(fn)

    def replayed():
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert graph.check() == 0
        return outs
    for a, b in zip(replayed(), want0):
        assert torch.equal(a, b)
    # structural changes raise and leave the arrays as they are
    held = [t.clone() for t in (rows.src, rows.w, rows.cnt)]
    with pytest.raises(ValueError):
        rows.set([[0, 1, 2], [1]]) if form == "mix" else rows.set([[0, 1], [1]])
    with pytest.raises(ValueError):
        rows.set([0, 3])  # not a voice of the bank
    assert all(torch.equal(a, b) for a, b in zip(held, (rows.src, rows.w, rows.cnt)))
    # other speakers (and, in the mix form, other weights) into the same arrays: the replay is the eager call
    want1 = eager(**other)
    assert not torch.equal(want1[0], want0[0])
    rows.set(**other)
    for a, b in zip(replayed(), want1):
        assert torch.equal(a, b)
    # a voice replaced in the bank, at the same addresses
    bank.replace(0, v_new)
    want2 = eager(**other)
    assert not torch.equal(want2[0], want1[0])
    for a, b in zip(replayed(), want2):
        assert torch.equal(a, b)
