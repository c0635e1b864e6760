"""Ragged reference batches through the prompt front end: prompt_features / prompt_encode with ref_lens
on SPEC_TINY, B = 4, the two batches of the design note -- N = 4500 with lengths [4500, 1025, 2999, 3000] and N = 39000
with [39000, 38400, 38399, 1025] -- on three engines: the default bf16 engine, the batch-1 latency engine (forked "enc"
site) and the precise front end (fp32 STFT / log-mel in one launch, split-operand convs).  Samples past a row's
length are NaN in every ragged input: a read would poison the row.

Row b of the ragged batch must compute what the same engine computes for ref_wav[b, :ref_lens[b]] alone: z at most
1e-6 of max|ref| (the _near rule of tests/test_gpu_ragged_stages.py; bit-identical is expected on both front ends and
which one it was is printed), the discrete codes equal.  The same rows are held against the CPU oracle run per row at
its own length at the bounds the uniform batch is held to: tests/test_gpu_frontend.py (z rel-L2 <= 3e-2, codes equal
wherever the oracle's decision margin exceeds the guard) for the bf16 front end, tests/test_gpu_precise_frontend.py
(z vs the fp64 restatement rel-L2 <= Z_REL_L2 = 2e-5 and max-abs <= 1e-4) for the precise one."""
import pytest
import torch

from refops import rel_err

pytestmark = pytest.mark.gpu

BATCHES = {"short": (4500, [4500, 1025, 2999, 3000]), "tile": (39000, [39000, 38400, 38399, 1025])}
ENGINES = ["default", "latency", "precise"]
TEXT_T, TEXT_LENS = 12, [12, 5, 9, 3]
STEPS, CFG = 2, 5.0


@pytest.fixture(scope="module")
def engines(gpu_device, tiny, tiny_params):
    """the three engines, built on first use"""
    from stzs.engine import StyleTTSZS, latency_engine
    made = {}

    def get(name):
        if name not in made:
            if name == "precise":
                made[name] = StyleTTSZS(tiny, tiny_params, device=gpu_device, precise_frontend=True)
            else:
                if "default" not in made:
                    made["default"] = StyleTTSZS(tiny, tiny_params, device=gpu_device)
                if name == "latency":
                    made[name] = latency_engine(tiny, made["default"].W, gpu_device)
        return made[name]
    return get


def _wav(batch, poisoned=True):
    N, lens = BATCHES[batch]
    wav = torch.randn(len(lens), N, generator=torch.Generator().manual_seed(N)) * 0.1
    if poisoned:
        for b, n in enumerate(lens):
            wav[b, n:] = float("nan")
    return wav


def _prompt(eng, wav, lens):
    """prompt_features and prompt_encode -> host copies (the engine's buffers are reused by the next call)"""
    dev = eng.device
    z = eng.prompt_features(wav.to(dev), lens).cpu().clone()
    q = eng.prompt_encode(wav.to(dev), ref_lens=lens).cpu().clone()
    return dict(z=z, q=q, idx=eng.prompt_idx.cpu().clone())


_runs = {}


def _ragged_and_solo(engines, name, batch):
    """the ragged batch and each row's solo run on one engine, computed once and shared"""
    if (name, batch) not in _runs:
        eng = engines(name)
        _, lens = BATCHES[batch]
        wav = _wav(batch)
        rag = _prompt(eng, wav, lens)
        solo = [_prompt(eng, wav[b:b + 1, :n], None) for b, n in enumerate(lens)]
        _runs[(name, batch)] = (rag, solo)
    return _runs[(name, batch)]


def _near(tag, got, want):
    """max-abs <= 1e-6 of max|ref|, the figure (or 'bit-identical') printed first"""
    got, want = got.float(), want.float()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err = ((got - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()
    print(f"  {tag}: " + ("bit-identical" if torch.equal(got, want) else f"max-abs / max|ref| = {err:.2e}"))
    assert err <= 1e-6, (tag, err)


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("name", ENGINES)
def test_ragged_rows_match_solo_runs(engines, name, batch):
    rag, solo = _ragged_and_solo(engines, name, batch)
    _, lens = BATCHES[batch]
    for k in ("z", "q"):
        assert bool(torch.isfinite(rag[k]).all()), k
    for b, n in enumerate(lens):
        print(f"{name} {batch} row {b} (n {n})")
        _near("z", rag["z"][b], solo[b]["z"][0])
        assert torch.equal(rag["idx"][b], solo[b]["idx"][0])
        assert torch.equal(rag["q"][b], solo[b]["q"][0])


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("name", ENGINES)
def test_ragged_rows_match_oracle(engines, tiny, tiny_params, name, batch):
    from oracle import stzs_ref as R
    S, P = tiny, tiny_params
    rag, _ = _ragged_and_solo(engines, name, batch)
    _, lens = BATCHES[batch]
    wav = _wav(batch)
    for b, n in enumerate(lens):
        one = wav[b:b + 1, :n]
        z = rag["z"][b:b + 1]
        if name == "precise":
            from test_gpu_precise_frontend import Z_REL_L2, _z64
            z64 = _z64(P, S, one)
            e, mx = rel_err(z.double(), z64), (z.double() - z64).abs().max().item()
            print(f"{name} {batch} row {b} (n {n}): rel-L2 {e:.3e} max-abs {mx:.3e} vs fp64")
            assert e <= Z_REL_L2
            assert mx <= 1e-4
        else:
            z_want = R.prompt_features(P, S, one)
            e = rel_err(z, z_want)
            _, idx_want, margin = R.prompt_encoder(P, S, one)
            guard = 4 * S.vq_group * (z - z_want).abs().max().item() * \
                (z_want.abs().max().item() + P["pe.vq"].abs().max().item())
            clear = margin > guard
            agree = rag["idx"][b:b + 1] == idx_want
            print(f"{name} {batch} row {b} (n {n}): rel-L2 {e:.3e} guard {guard:.3e} clear "
                  f"{clear.float().mean().item():.3f} agree {agree.float().mean().item():.3f}")
            assert e <= 3e-2
            assert bool(agree[clear].all())
        assert torch.equal(rag["q"][b:b + 1], R.lookup_codes(P, S, rag["idx"][b:b + 1]))


@pytest.mark.parametrize("name", ["default", "precise"])
def test_host_list_and_device_tensor_give_the_same_bits(engines, name):
    eng = engines(name)
    rag, _ = _ragged_and_solo(engines, name, "short")
    _, lens = BATCHES["short"]
    dev_lens = torch.tensor(lens, dtype=torch.int32, device=eng.device)
    got = _prompt(eng, _wav("short"), dev_lens)
    for k in ("z", "q", "idx"):
        assert torch.equal(got[k], rag[k]), k
    host_tensor = _prompt(eng, _wav("short"), torch.tensor(lens))
    assert torch.equal(host_tensor["z"], rag["z"])
    with pytest.raises(ValueError):
        eng.prompt_features(_wav("short").to(eng.device), [4500, 1024, 2999, 3000])  # below n_fft / 2 + 1
    with pytest.raises(ValueError):
        eng.prompt_features(_wav("short").to(eng.device), dev_lens[:3])  # one length per row


@pytest.mark.parametrize("name", ["default", "precise"])
def test_uniform_call_after_a_ragged_one(engines, name):
    """ref_lens=None after a ragged call on the same buffers: the uniform result (nothing stale is read), which is
    also the ragged call with every length N"""
    eng = engines(name)
    N, lens = BATCHES["short"]
    clean = _wav("short", poisoned=False)
    before = _prompt(eng, clean, None)
    _prompt(eng, _wav("short"), lens)
    after = _prompt(eng, clean, None)
    full = _prompt(eng, clean, [N] * len(lens))
    for k in ("z", "q", "idx"):
        assert torch.equal(after[k], before[k]), k
        assert torch.equal(full[k], before[k]), k
    # prompt_idx given: the reference and its lengths are ignored
    q = eng.prompt_encode(None, prompt_idx=before["idx"].to(eng.device), ref_lens=[1, 2, 3]).cpu()
    assert torch.equal(q, before["q"])


@pytest.mark.parametrize("name", ENGINES)
def test_text_and_reference_ragged_together(engines, tiny, name):
    """text_lens [12, 5, 9, 3] with the first reference batch through encode_inputs (the forked site on the latency
    engine), sample_style and predict_durations: codes, d and dur of row b equal the solo run of that row at its own
    token count and its own reference length"""
    S = tiny
    eng = engines(name)
    dev = eng.device
    _, rl = BATCHES["short"]
    g = torch.Generator().manual_seed(4321)
    tok = torch.randint(1, S.n_symbols, (4, TEXT_T), generator=g)
    eps = torch.randn(4, S.L_s, S.code_dim, generator=g)
    wav = _wav("short")

    def front(tok, wav, eps, tl, rlens):
        h, prompt = eng.encode_inputs(tok.to(dev, torch.int32), wav.to(dev), None, tl, rlens)
        codes = eng.sample_style(h, prompt, eps.to(dev), STEPS, CFG, tl)
        du = eng.predict_durations(h, codes, None, tl)
        assert eng.check_status() == 0
        return dict(codes=codes.cpu().clone(), d=du["d"].t[:, :, :S.pr_in].cpu().clone(), dur=du["dur"].cpu().clone(),
                    idx=eng.prompt_idx.cpu().clone())
    rag = front(tok, wav, eps, TEXT_LENS, rl)
    for b, (n, m) in enumerate(zip(TEXT_LENS, rl)):
        one = front(tok[b:b + 1, :n], wav[b:b + 1, :m], eps[b:b + 1], None, None)
        for k, got in (("codes", rag["codes"][b]), ("d", rag["d"][b, :n]), ("dur", rag["dur"][b, :n])):
            want = one[k][0]
            err = ((got.float() - want.float()).abs().max() / want.float().abs().max().clamp_min(1e-30)).item()
            print(f"{name} row {b} (tokens {n}, samples {m}) {k}: " +
                  ("bit-identical" if torch.equal(got, want) else f"max-abs / max|ref| = {err:.2e}"))
            assert torch.equal(got, want), (k, b, err)
        assert torch.equal(rag["idx"][b], one["idx"][0])
        assert bool((rag["dur"][b, n:] == 0).all())


def test_ragged_front_captures(gpu_device, tiny, tiny_params):
    """the front with text_lens and ref_lens as device tensors is capturable (no host sync, no upload: the frame
    counts come from the STFT launch) and its replay equals the eager result"""
    from stzs.engine import StyleTTSZS
    S = tiny
    eng = StyleTTSZS(S, tiny_params, device=gpu_device)  # (its own buffer cache: a capture pins its shapes)
    _, rl = BATCHES["short"]
    g = torch.Generator().manual_seed(4321)
    tokd = torch.randint(1, S.n_symbols, (4, TEXT_T), generator=g).to(gpu_device, torch.int32)
    epsd = torch.randn(4, S.L_s, S.code_dim, generator=g).to(gpu_device)
    refd = _wav("short").to(gpu_device)
    tl = torch.tensor(TEXT_LENS, dtype=torch.int32, device=gpu_device)
    rlens = torch.tensor(rl, dtype=torch.int32, device=gpu_device)

    def front():
        h, prompt = eng.encode_inputs(tokd, refd, None, tl, rlens)
        codes = eng.sample_style(h, prompt, epsd, STEPS, CFG, tl)
        du = eng.predict_durations(h, codes, None, tl)
        return prompt, eng.prompt_idx, codes, du["d"].t, du["dur"]

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
    assert bool(torch.isfinite(outs[0]).all())
