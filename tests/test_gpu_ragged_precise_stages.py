"""Ragged frames and the ragged decoder on the PRECISE engines, through the engine.  Spec and shapes of
tests/test_gpu_ragged_decoder_stages.py: SPEC_TINY with dec_out 128 and gen_ch (256, 128), B = 4 rows of forced
[7, 1, 3, 6] frames, text lengths [12, 5, 9, 3].  Engines: precise=True (every conv on the mrfx / conv_x3 forms),
precise_decoder=True (bf16 front, fp32 decoder) and precise=True with the mrfx switch off (every conv on conv_x3).

Row b of the ragged batch must be, bit for bit, what the SAME engine computes for that row alone at T40 = T_b: the
prosody (idx, en, aligned text, F0[b, :2 T_b], N[b, :2 T_b]), every traced decoder stage's valid rows and
wav[b, :600 T_b]; the waveform tail is exact zeros.  One oracle test at v0 holds each row of a ragged batch to the
row-alone fp32 oracle at the north-star bound (log-mel L1 <= 1e-3)."""
import pytest
import torch

from test_gpu_ragged_decoder_stages import B, CFG, FRAMES, STEPS, T, TEXT_LENS, _check, _decode, _h_act, _inputs, _split
from test_gpu_ragged_stream_stages import CHUNK, HALO, _cat, _synth_inputs

pytestmark = pytest.mark.gpu

ENGINES = {"precise": (dict(precise=True), True), "precise_decoder": (dict(precise_decoder=True), True),
           "precise_x3": (dict(precise=True), False)}


@pytest.fixture(scope="module")
def spec(tiny):
    return tiny.replace(dec_out=128, gen_ch=(256, 128))


@pytest.fixture(scope="module")
def params(spec):
    from stzs.params import init_params
    return init_params(spec, seed=2)


@pytest.fixture(scope="module")
def engines(gpu_device, spec, params):
    from stzs.engine import StyleTTSZS
    out = {}
    for name, (kw, mrfx) in ENGINES.items():
        e = StyleTTSZS(spec, params, device=gpu_device, **kw)
        e.mrfx = mrfx and e.mrfx
        e._check_ragged_frames()
        e._check_ragged_decoder()
        out[name] = e
    return out


def _pro_host(S, pro):
    return dict(idx=pro["idx"].cpu().clone(), en=pro["en"].t[:, :, :S.pr_in].float().cpu().clone(),
                asr=pro["asr_buf"].t[:, :, :S.d_txt].float().cpu().clone(), F0=pro["F0"].cpu().clone(),
                N=pro["N"].cpu().clone(), T40=pro["T40"])


@pytest.mark.parametrize("name", list(ENGINES))
def test_prosody_rows_match_solo(engines, spec, name):
    eng, S = engines[name], spec
    h, codes = _inputs(S)
    dur = torch.tensor([_split(n) for n in FRAMES], dtype=torch.int32)
    cd = codes.to(eng.device)
    pro = eng.predict_prosody(_h_act(eng, h), cd, dur, ragged_frames=True)
    assert pro["frame_lens"].cpu().tolist() == FRAMES and pro["T40"] == max(FRAMES)
    rag = _pro_host(S, pro)
    assert bool(torch.isfinite(rag["F0"]).all()) and bool(torch.isfinite(rag["N"]).all())
    for b, n in enumerate(FRAMES):
        one = _pro_host(S, eng.predict_prosody(_h_act(eng, h[b:b + 1]), cd[b:b + 1], dur[b:b + 1]))
        assert one["T40"] == n
        for k, m in (("idx", 1), ("en", 1), ("asr", 1), ("F0", 2), ("N", 2)):
            assert torch.equal(rag[k][b, :m * n], one[k][0]), f"{name}: row {b} ({n} frames): {k} differs from its solo run"
    assert eng.check_status() == 0


@pytest.mark.parametrize("name", list(ENGINES))
def test_decode_rows_match_solo(engines, spec, name):
    """decode(frame_lens=...) with the trace: every stage's valid rows and the waveform, tails finite / exact zeros"""
    eng, S = engines[name], spec
    h, codes = _inputs(S)
    dur = torch.tensor([_split(n) for n in FRAMES], dtype=torch.int32)
    rag = _decode(eng, S, h, codes, dur, [10, 11, 12, 13], True)
    solos = [_decode(eng, S, h[b:b + 1], codes[b:b + 1], dur[b:b + 1], [10 + b], False) for b in range(B)]
    assert eng.check_status() == 0
    _check(S, rag, solos, FRAMES)


def test_synth_with_per_row_speed_matches_solo(engines, spec):
    """free-running synth(ragged_frames=True), ragged text and references, each row at its own speaking rate"""
    eng, S = engines["precise"], spec
    tok, ref, eps, rl, _ = _synth_inputs(S)
    speed = [1.0, 0.8, 1.25, 1.0]
    wav, fl = eng.synth(tok, ref, steps=STEPS, cfg_scale=CFG, noise=eps, seeds=[3, 4, 5, 6], text_lens=TEXT_LENS,
                        ref_lens=rl, ragged_frames=True, controls=eng.row_controls(B, speed=speed))
    wav, fl = wav.cpu().clone(), fl.cpu().tolist()
    print("predicted frame counts", fl)
    assert wav.shape == (B, S.frame40 * max(fl)) and bool(torch.isfinite(wav).all())
    for b, n in enumerate(TEXT_LENS):
        one = eng.synth(tok[b:b + 1, :n], ref[b:b + 1, :rl[b]], steps=STEPS, cfg_scale=CFG, noise=eps[b:b + 1],
                        seeds=[3 + b], controls=eng.row_controls(1, speed=speed[b]))["wav"].cpu()
        assert one.shape == (1, S.frame40 * fl[b]), (one.shape, fl[b])
        assert torch.equal(wav[b, :one.shape[1]], one[0]), f"row {b} differs from its solo synth()"
        assert bool((wav[b, one.shape[1]:] == 0).all()), f"row {b}: the tail is not exact zeros"


def test_synth_stream_concatenates_to_the_ragged_synth(engines, spec):
    """synth_stream(ragged_frames=True): the exact stream's chunks tile the ragged synth(); with chunked_halo every row
    is its own chunked stream alone"""
    eng, S = engines["precise"], spec
    tok, ref, eps, rl, dur = _synth_inputs(S)
    chunk_s = CHUNK * S.frame40 / S.sr
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[3, 4, 5, 6], text_lens=TEXT_LENS, ref_lens=rl)
    width = S.frame40 * max(FRAMES)
    wav, _ = _cat(eng.synth_stream(tok, ref, chunk_s=chunk_s, ragged_frames=True, **kw), width)
    whole, fl = eng.synth(tok, ref, ragged_frames=True, **kw)
    assert fl.cpu().tolist() == FRAMES
    assert torch.equal(wav, whole.cpu()), "the concatenated chunks differ from synth(ragged_frames=True)"
    got, _ = _cat(eng.synth_stream(tok, ref, chunk_s=chunk_s, chunked_halo=HALO, ragged_frames=True, **kw), width)
    for b, (n, tl) in enumerate(zip(FRAMES, TEXT_LENS)):
        solo, _ = _cat(eng.synth_stream(tok[b:b + 1, :tl], ref[b:b + 1, :rl[b]], steps=STEPS, cfg_scale=CFG,
                                        noise=eps[b:b + 1], durations=dur[b:b + 1, :tl], seeds=[3 + b], chunk_s=chunk_s,
                                        chunked_halo=HALO), S.frame40 * n)
        assert torch.equal(got[b, :S.frame40 * n], solo[0]), f"row {b} ({n} frames) differs from its solo chunked stream"
        assert bool((got[b, S.frame40 * n:] == 0).all()), f"row {b}: the tail is not exact zeros"


def test_captured_synth_replays_to_the_same_bits(gpu_device, spec, params, engines):
    """synth() with n_frames and device lengths makes no host sync: captured, its replay equals the eager result"""
    from stzs.engine import StyleTTSZS
    S = spec
    e2 = StyleTTSZS(S, params, device=gpu_device, precise=True)  # (its own buffer cache: a capture pins its shapes)
    tok, ref, eps, rl, dur = _synth_inputs(S)
    dev = gpu_device
    tl = torch.tensor(TEXT_LENS, dtype=torch.int32, device=dev)
    rld = torch.tensor(rl, dtype=torch.int32, device=dev)
    tokd, refd, epsd, durd = tok.to(dev), ref.to(dev), eps.to(dev), dur.to(dev)
    seeds = torch.tensor([3, 4, 5, 6], dtype=torch.int32, device=dev)

    def run():
        return e2.synth(tokd, refd, steps=STEPS, cfg_scale=CFG, noise=epsd, durations=durd, seeds=seeds, text_lens=tl,
                        ref_lens=rld, n_frames=max(FRAMES), ragged_frames=True, check=False)[0]

    eager = run().clone()
    graph, out = e2.capture(run)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert graph.check() == 0
    assert torch.equal(out, eager)
    want, _ = engines["precise"].synth(tok, ref, steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[3, 4, 5, 6],
                                       text_lens=TEXT_LENS, ref_lens=rl, ragged_frames=True)
    assert torch.equal(eager, want)


def test_branch_streams_give_the_same_bits(gpu_device, spec, params, engines):
    from stzs.engine import StyleTTSZS
    S = spec
    h, codes = _inputs(S)
    dur = torch.tensor([_split(n) for n in FRAMES], dtype=torch.int32)
    ref_ = _decode(engines["precise"], S, h, codes, dur, [10, 11, 12, 13], True)
    e2 = StyleTTSZS(S, params, device=gpu_device, precise=True, branch_streams=True)
    got = _decode(e2, S, h, codes, dur, [10, 11, 12, 13], True)
    assert e2.check_status() == 0
    assert torch.equal(got[0], ref_[0]), "branch_streams=True changes the ragged waveform"
    for k in ref_[1]:
        assert torch.equal(got[1][k], ref_[1][k]), k


def test_still_refused(gpu_device, spec, params, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    e = StyleTTSZS(spec, params, device=gpu_device, precise=True)
    e.blk_splitk = 4
    with pytest.raises(NotImplementedError):
        e._check_ragged_decoder()
    with pytest.raises(NotImplementedError):
        StyleTTSZS(tiny, tiny_params, device=gpu_device)._check_ragged_decoder()  # (generic-path bf16 generator convs)


# ---- against the oracle, at v0 ---------------------------------------------------------------------------------------

def test_ragged_rows_meet_the_north_star_at_v0(gpu_device):
    """the v0_precise construction of tests/test_gpu_precise.py (SPEC_V0, init_params seed 0, precise=True), B = 3 rows of
    different forced frame counts (>= 3 frames: the oracle's instance norm), prompt codes teacher-forced: each row of
    synth(ragged_frames=True) against the row-alone oracle, log-mel L1 <= 1e-3 (the bound test_precise_end_to_end_mel_l1
    asserts)"""
    from oracle import stzs_ref as R
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.spec import SPEC_V0 as S
    torch.set_num_threads(16)
    P = init_params(S, seed=0)
    eng = StyleTTSZS(S, P, device=gpu_device, precise=True)
    g = torch.Generator().manual_seed(7)
    Bv, Tv, frames = 3, 8, [12, 5, 9]
    tok = torch.randint(1, S.n_symbols, (Bv, Tv), generator=g)
    ref = torch.randn(Bv, S.sr // 2, generator=g) * 0.1
    eps = torch.randn(Bv, S.L_s, S.code_dim, generator=g)
    dur = torch.tensor([_split(n, Tv) for n in frames], dtype=torch.int32)
    wav, fl = eng.synth(tok, ref, steps=2, cfg_scale=5.0, noise=eps, durations=dur, seeds=[0, 1, 2], ragged_frames=True)
    assert fl.cpu().tolist() == frames
    wav, pidx = wav.cpu(), eng.prompt_idx.cpu()
    for b, n in enumerate(frames):
        o = R.synth(P, S, tok[b:b + 1], ref[b:b + 1], 2, 5.0, eps[b:b + 1], dur[b:b + 1], seeds=[b],
                    prompt_idx=pidx[b:b + 1])
        m = (R.log_mel(wav[b:b + 1, :S.frame40 * n], S) - R.log_mel(o["wav"], S)).abs().mean().item()
        print(f"v0 ragged row {b} ({n} frames): log-mel L1 {m:.3e}")
        assert o["wav"].shape == (1, S.frame40 * n) and m <= 1e-3, (b, m)
        assert bool((wav[b, S.frame40 * n:] == 0).all())
