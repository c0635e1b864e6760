"""Ragged text batches through the stages (DESIGN.md "Ragged text batches"): text_encode -> prompt_encode ->
sample_style -> predict_durations with text_lens on SPEC_TINY, B = 4 rows padded to T = 12 with lengths
[12, 5, 9, 3], 2 steps, CFG 5, on three engines: the default bf16 engine, the batch-1 latency engine and the
precise (split-operand fp32) engine.

Row b of the ragged batch must compute what the same engine computes for that row alone at T = text_lens[b]:
max-abs <= 1e-6 of max|ref| (tests/test_gpu_scheduler.py's bound; bit-identical is expected and which one it was is
printed), durations exactly equal, padding as documented (h_txt rows and durations 0).  The same rows are also held
against the CPU oracle, run per row at its own length, at the bounds of tests/test_gpu_stages.py (text encoder
rel-L2 1.2e-2 free-running, 2-step CFG-5 sampler 2e-2 and the duration sum 0.15 abs / durations equal outside the
tie window, both teacher-forced with the oracle's text rows and the GPU's prompt codes); the precise engine is held
to the same bounds (tests/test_gpu_precise.py asserts none of its own on these stage outputs) and its far smaller
figures are printed."""
import pytest
import torch

from refops import rel_err

pytestmark = pytest.mark.gpu

B, T, LENS = 4, 12, [12, 5, 9, 3]
STEPS, CFG = 2, 5.0
ENGINES = ["default", "latency", "precise"]


def _inputs(S):
    g = torch.Generator().manual_seed(4321)
    tok = torch.randint(1, S.n_symbols, (B, T), generator=g)
    ref = torch.randn(B, S.sr, generator=g) * 0.1
    eps = torch.randn(B, S.L_s, S.code_dim, generator=g)
    return tok, ref, eps


@pytest.fixture(scope="module")
def engines(gpu_device, tiny, tiny_params):
    """the three engines, built on first use"""
    from stzs.engine import StyleTTSZS, latency_engine
    made = {}

    def get(name):
        if name not in made:
            if name == "precise":
                made[name] = StyleTTSZS(tiny, tiny_params, device=gpu_device, precise=True)
            else:
                if "default" not in made:
                    made["default"] = StyleTTSZS(tiny, tiny_params, device=gpu_device)
                if name == "latency":
                    made[name] = latency_engine(tiny, made["default"].W, gpu_device)
        return made[name]
    return get


def _front(eng, S, tok, ref, eps, lens):
    """the four stages on device inputs -> their outputs as host copies (the engine's buffers are reused by the next
    call); lens: None, a host list or an int32 device tensor"""
    dev = eng.device
    h = eng.text_encode(tok.to(dev, torch.int32), lens)
    prompt = eng.prompt_encode(ref.to(dev))
    codes = eng.sample_style(h, prompt, eps.to(dev), STEPS, CFG, lens)
    du = eng.predict_durations(h, codes, None, lens)
    assert eng.check_status() == 0
    return dict(h=h.t[:, :, :S.d_txt].cpu().clone(), codes=codes.cpu().clone(),
                d=du["d"].t[:, :, :S.pr_in].cpu().clone(), dur=du["dur"].cpu().clone(),
                dsum=du["dsum"].cpu().clone(), logits=du["logits"].t.cpu().clone(),
                prompt_idx=eng.prompt_idx.cpu().clone())


_runs = {}


def _ragged_and_solo(engines, name, S):
    """the ragged batch and each row's solo run on one engine, computed once per engine and shared"""
    if name not in _runs:
        eng = engines(name)
        tok, ref, eps = _inputs(S)
        rag = _front(eng, S, tok, ref, eps, LENS)
        solo = [_front(eng, S, tok[b:b + 1, :n], ref[b:b + 1], eps[b:b + 1], None) for b, n in enumerate(LENS)]
        _runs[name] = (rag, solo)
    return _runs[name]


def _near(tag, got, want):
    """max-abs <= 1e-6 of max|ref|, the figure (or 'equal') printed first"""
    got, want = got.float(), want.float()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err = ((got - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()
    print(f"  {tag}: " + ("bit-identical" if torch.equal(got, want) else f"max-abs / max|ref| = {err:.2e}"))
    assert err <= 1e-6, (tag, err)


@pytest.mark.parametrize("name", ENGINES)
def test_ragged_rows_match_solo_runs(engines, tiny, name):
    S = tiny
    rag, solo = _ragged_and_solo(engines, name, S)
    for b, n in enumerate(LENS):
        one = solo[b]
        print(f"{name} row {b} (len {n})")
        assert torch.equal(rag["prompt_idx"][b], one["prompt_idx"][0])
        _near("h_txt", rag["h"][b, :n], one["h"][0])
        _near("codes", rag["codes"][b], one["codes"][0])
        _near("d", rag["d"][b, :n], one["d"][0])
        assert torch.equal(rag["dur"][b, :n], one["dur"][0]), (b, rag["dur"][b], one["dur"][0])
        assert bool((rag["dur"][b, :n] >= 1).all())
        # the documented padding: h_txt rows and durations 0, the unspecified ones finite
        assert bool((rag["h"][b, n:] == 0).all()) and bool((rag["dur"][b, n:] == 0).all())
    for k in ("d", "logits", "dsum", "codes"):
        assert bool(torch.isfinite(rag[k].float()).all()), k


def _act(eng, x):
    from stzs.engine import Act
    t = torch.zeros(*x.shape, dtype=eng.adt, device=eng.device)
    t.copy_(x.to(eng.adt))
    return Act(t)


@pytest.mark.parametrize("name", ENGINES)
def test_ragged_rows_match_oracle(engines, tiny, tiny_params, name):
    from oracle import stzs_ref as R
    S, P = tiny, tiny_params
    eng = engines(name)
    rag, _ = _ragged_and_solo(engines, name, S)
    tok, ref, eps = _inputs(S)
    lowp = eng.adt != torch.float32
    rnd = (lambda v: v.to(torch.bfloat16).float()) if lowp else (lambda v: v)
    # text encoder, free-running from the tokens
    h_ref = [R.text_encoder(P, S, tok[b:b + 1, :n]) for b, n in enumerate(LENS)]
    for b, n in enumerate(LENS):
        e = rel_err(rag["h"][b:b + 1, :n].float(), h_ref[b])
        print(f"{name} row {b} (len {n}): text rel-L2 {e:.2e}")
        assert e < 1.2e-2
    # sampler and durations, teacher-forced: the oracle's text rows (as the engine stores them) padded with zeros,
    # the GPU's prompt codes
    hp = torch.zeros(B, T, S.d_txt)
    for b, n in enumerate(LENS):
        hp[b, :n] = rnd(h_ref[b][0])
    prompt = R.prompt_encoder(P, S, ref, prompt_idx=rag["prompt_idx"])[0]
    dev = eng.device
    codes = eng.sample_style(_act(eng, hp), prompt.to(dev), eps.to(dev), STEPS, CFG, LENS).cpu()
    cin = torch.randn(B, S.L_s, S.code_dim, generator=torch.Generator().manual_seed(3)) * 0.3
    du = eng.predict_durations(_act(eng, hp), cin.to(dev), None, LENS)
    dsum, dur = du["dsum"].cpu(), du["dur"].cpu()
    assert eng.check_status() == 0
    for b, n in enumerate(LENS):
        c_ref = R.sample_style(P, S, hp[b:b + 1, :n], prompt[b:b + 1], eps[b:b + 1], STEPS, CFG)
        e = rel_err(codes[b:b + 1], c_ref)
        pr = R.predict_prosody(P, S, hp[b:b + 1, :n], cin[b:b + 1])
        e_dsum = (dsum[b:b + 1, :n] - pr["dur_sum"]).abs().max().item()
        tie = (pr["dur_sum"] - pr["dur_sum"].floor() - 0.5).abs() <= e_dsum + 1e-4
        print(f"{name} row {b} (len {n}): sampler rel-L2 {e:.2e}, dsum max abs {e_dsum:.2e}, "
              f"guarded ties {int(tie.sum())} of {tie.numel()}")
        assert e < 2e-2
        assert e_dsum < 0.15
        assert bool(((dur[b:b + 1, :n] == pr["dur_pred"]) | tie).all())
        assert bool((dur[b, n:] == 0).all())


def test_ragged_front_captures(gpu_device, tiny, tiny_params):
    """the ragged front with text_lens as a device tensor is capturable (no host sync, no upload) and its replay
    equals the eager result; graph.check() reads a clean status word"""
    from stzs.engine import StyleTTSZS
    S = tiny
    eng = StyleTTSZS(S, tiny_params, device=gpu_device)  # (its own buffer cache: a capture pins its shapes)
    tok, ref, eps = _inputs(S)
    tokd, refd, epsd = tok.to(gpu_device, torch.int32), ref.to(gpu_device), eps.to(gpu_device)
    lens = torch.tensor(LENS, dtype=torch.int32, device=gpu_device)

    def front():
        h = eng.text_encode(tokd, lens)
        codes = eng.sample_style(h, eng.prompt_encode(refd), epsd, STEPS, CFG, lens)
        du = eng.predict_durations(h, codes, None, lens)
        return h.t, codes, du["d"].t, du["dur"]

    eager = [t.clone() for t in front()]
    assert eng.check_status() == 0
    graph, outs = eng.capture(front)
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert graph.check() == 0
    for k, (a, b) in enumerate(zip(outs, eager)):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("name", ["default", "latency"])
def test_ragged_synth_with_forced_durations(engines, tiny, name):
    """synth(text_lens=...) end to end on a batch that shares its frame count (24): lengths [8, 5], forced durations
    whose padding entries are NOT zero (the engine must not count or align them) -- the duration LSTM runs paired with
    the shared LSTM (stzs_lstm_pair with its own lens).  Every waveform within 1e-6 of the row's solo synth()."""
    S = tiny
    eng = engines(name)
    g = torch.Generator().manual_seed(77)
    lens = [8, 5]
    tok = torch.randint(1, S.n_symbols, (2, 8), generator=g)
    ref = torch.randn(2, S.sr, generator=g) * 0.1
    eps = torch.randn(2, S.L_s, S.code_dim, generator=g)
    dur = torch.tensor([[3] * 8, [5, 5, 5, 5, 4, 9, 9, 9]], dtype=torch.int32)
    out = eng.synth(tok, ref, steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[3, 4], text_lens=lens)
    wav, dur_out = out["wav"].clone(), out["dur"].cpu().clone()
    assert wav.shape[1] == 24 * S.frame40
    assert dur_out.tolist() == [[3] * 8, [5, 5, 5, 5, 4, 0, 0, 0]]
    for b, n in enumerate(lens):
        one = eng.synth(tok[b:b + 1, :n], ref[b:b + 1], steps=STEPS, cfg_scale=CFG, noise=eps[b:b + 1],
                        durations=dur[b:b + 1, :n], seeds=[3 + b])["wav"][0]
        err = ((wav[b] - one).abs().max() / one.abs().max()).item()
        print(f"{name} row {b} (len {n}):", "equal" if torch.equal(wav[b], one) else f"max-rel {err:.2e}")
        assert err <= 1e-6


def test_ragged_scheduler_matches_single_requests(engines, tiny):
    """the request mix of tests/test_gpu_scheduler.py on BucketScheduler(ragged_text=True): every waveform within
    1e-6 of its solo synth(), in as many phase-1 batches as phase1_groups says -- fewer than without ragged_text"""
    from stzs.scheduler import BucketScheduler, Request
    S = tiny
    eng = engines("default")
    g = torch.Generator().manual_seed(21)
    reqs = []
    for k, (Tn, nref, forced) in enumerate([(8, S.sr, None), (12, S.sr, None), (12, S.sr, None),
                                            (8, S.sr + S.sr // 2, None), (10, S.sr, [4] * 10), (8, S.sr, [5] * 8),
                                            (6, S.sr, None)]):
        reqs.append(Request(tokens=torch.randint(1, S.n_symbols, (Tn,), generator=g),
                            ref_wav=torch.randn(nref, generator=g) * 0.1,
                            noise=torch.randn(S.L_s, S.code_dim, generator=g), seed=100 + k,
                            durations=torch.tensor(forced, dtype=torch.int32) if forced else None))
    sch = BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG, ragged_text=True)
    outs = sch.synth(reqs)
    print("ragged scheduler", sch.stats)
    n_ragged = len(sch.phase1_groups(reqs))
    n_plain = len(BucketScheduler(eng, max_batch=4, steps=STEPS, cfg_scale=CFG).phase1_groups(reqs))
    assert sch.stats["phase1_batches"] == n_ragged == 3 and n_ragged < n_plain == 6
    for r, w in zip(reqs, outs):
        one = eng.synth(r.tokens[None], r.ref_wav[None], steps=STEPS, cfg_scale=CFG, noise=r.noise[None],
                        durations=r.durations[None] if r.durations is not None else None, seeds=[r.seed])["wav"][0]
        assert w.shape == one.shape
        err = ((w - one).abs().max() / one.abs().max()).item()
        print("len", w.shape[0], "equal" if torch.equal(w, one) else f"max-rel {err:.2e}")
        assert err <= 1e-6
