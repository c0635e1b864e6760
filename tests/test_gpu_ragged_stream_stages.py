"""Ragged streaming through the engine: synth_stream(ragged_frames=True), with and without the chunked
decoder, and decode_chunked(frame_lens=...), on the smallest spec that passes _check_ragged_decoder (SPEC_TINY with
dec_out 128 and gen_ch (256, 128), as tests/test_gpu_ragged_decoder_stages.py).

B = 4 rows with forced durations of [7, 1, 3, 6] frames, streamed in chunks of 2 aligned frames (240 iSTFT frames, 1200
samples): row 1 ends inside the first chunk, row 2 inside the second, row 3 (6 frames) exactly on the third chunk's
boundary -- its last iSTFT frame (720) is read by the fourth chunk's launch and its last samples are finalised there --
and row 0 in the 1-frame fourth chunk.  Every check is bit equality against what the same engine computes for the row
alone; the tails are exact zeros."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T = 4, 12
FRAMES = [7, 1, 3, 6]
TEXT_LENS = [12, 5, 9, 3]
STEPS, CFG = 2, 5.0
CHUNK, HALO = 2, 1


@pytest.fixture(scope="module")
def spec(tiny):
    return tiny.replace(dec_out=128, gen_ch=(256, 128))


@pytest.fixture(scope="module")
def params(spec):
    from stzs.params import init_params
    return init_params(spec, seed=2)


@pytest.fixture(scope="module")
def eng(gpu_device, spec, params):
    from stzs.engine import StyleTTSZS
    e = StyleTTSZS(spec, params, device=gpu_device)
    e._check_ragged_decoder()
    return e


def _split(n, T=T):
    return [n // T + (1 if t < n % T else 0) for t in range(T)]


def _cat(gen, width=None):
    """the chunks of a stream -> (host waveform, [(first sample, samples)]); the chunks must tile from 0"""
    spans, parts, end = [], [], 0
    for n0, w in gen:
        assert n0 == end, (n0, end)
        end = n0 + w.shape[1]
        spans.append((n0, w.shape[1]))
        parts.append(w)
    wav = torch.cat(parts, 1).cpu().clone()
    if width is not None:
        assert end == width, (end, width)
    return wav, spans


def _h_act(eng, h):
    from stzs.engine import Act
    t = torch.zeros(*h.shape, dtype=eng.adt, device=eng.device)
    t.copy_(h.to(eng.adt))
    return Act(t)


# ---- synth_stream ----------------------------------------------------------------------------------------------------

def _synth_inputs(S):
    g = torch.Generator().manual_seed(31)
    tok = torch.randint(1, S.n_symbols, (B, T), generator=g)
    N = S.sr // 2
    ref = torch.randn(B, N, generator=g) * 0.1
    eps = torch.randn(B, S.L_s, S.code_dim, generator=g)
    rl = [N, 7 * N // 10 + 1, N, S.mel_nfft // 2 + 1]
    dur = torch.zeros(B, T, dtype=torch.int32)
    for b, (n, tl) in enumerate(zip(FRAMES, TEXT_LENS)):
        dur[b, :tl] = torch.tensor(_split(n, tl), dtype=torch.int32)
    return tok, ref, eps, rl, dur


def test_synth_stream_ragged_frames(eng, spec):
    S = spec
    tok, ref, eps, rl, dur = _synth_inputs(S)
    chunk_s = CHUNK * S.frame40 / S.sr
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[3, 4, 5, 6], text_lens=TEXT_LENS, ref_lens=rl)
    width = S.frame40 * max(FRAMES)
    eng.frame_lens = None
    it = eng.synth_stream(tok, ref, chunk_s=chunk_s, ragged_frames=True, **kw)
    first = next(it)
    assert eng.frame_lens is not None and eng.frame_lens.cpu().tolist() == FRAMES  # from the first yield on
    wav, spans = _cat((c for c in [first] + list(it)), width)
    assert spans == [(0, 1190), (1190, 1200), (2390, 1200), (3590, 610)]  # the spans of the padded width
    whole, fl = eng.synth(tok, ref, ragged_frames=True, **kw)
    assert fl.cpu().tolist() == FRAMES
    assert torch.equal(wav, whole.cpu()), "the concatenated chunks differ from synth(ragged_frames=True)"
    assert bool(torch.isfinite(wav).all())
    for b, (n, tl) in enumerate(zip(FRAMES, TEXT_LENS)):
        solo, _ = _cat(eng.synth_stream(tok[b:b + 1, :tl], ref[b:b + 1, :rl[b]], steps=STEPS, cfg_scale=CFG,
                                        noise=eps[b:b + 1], durations=dur[b:b + 1, :tl], seeds=[3 + b],
                                        chunk_s=chunk_s), S.frame40 * n)
        assert torch.equal(wav[b, :S.frame40 * n], solo[0]), f"row {b} ({n} frames) differs from its solo stream"
        assert bool((wav[b, S.frame40 * n:] == 0).all()), f"row {b}: the tail is not exact zeros"


# ---- decode_chunked --------------------------------------------------------------------------------------------------

_runs = {}


def _chunked(eng, S):
    """ragged prosody of the forced rows, the rows' own copies of it, and the ragged chunked decode (host lengths)"""
    if "c" not in _runs:
        dev = eng.device
        g = torch.Generator().manual_seed(99)
        h = torch.randn(B, T, S.d_txt, generator=g).to(torch.bfloat16).float()
        codes = (torch.randn(B, S.L_s, S.code_dim, generator=g) * 0.3).to(dev)
        dur = torch.tensor([_split(n) for n in FRAMES], dtype=torch.int32)
        pro = eng.predict_prosody(_h_act(eng, h), codes, dur, ragged_frames=True)
        assert pro["T40"] == max(FRAMES)
        solo_pro = [eng.prosody_rows(pro, [b], n) for b, n in enumerate(FRAMES)]
        seeds = [10, 11, 12, 13]
        l0 = eng.launches
        rag, spans = _cat(eng.decode_chunked(pro, codes, seeds, CHUNK, HALO, frame_lens=FRAMES), S.frame40 * max(FRAMES))
        _runs["c"] = (pro, codes, seeds, solo_pro, rag, spans, eng.launches - l0)
    return _runs["c"]


def test_decode_chunked_rows_match_solo(eng, spec):
    S = spec
    pro, codes, seeds, solo_pro, rag, spans, launches = _chunked(eng, S)
    print("ragged chunked decode: launches", launches, "spans", spans)
    assert len(spans) == 4 and bool(torch.isfinite(rag).all())
    for b, n in enumerate(FRAMES):
        solo, _ = _cat(eng.decode_chunked(solo_pro[b], codes[b:b + 1], seeds[b:b + 1], CHUNK, HALO), S.frame40 * n)
        assert torch.equal(rag[b, :S.frame40 * n], solo[0]), f"row {b} ({n} frames) differs from its solo decode_chunked"
        assert bool((rag[b, S.frame40 * n:] == 0).all()), f"row {b}: the tail is not exact zeros"
    assert eng.check_status() == 0


@pytest.mark.parametrize("kw", [dict(batch_windows=False), dict(max_pass_rows=4)], ids=["one_by_one", "pass_rows_4"])
def test_decode_chunked_pass_split_keeps_the_bits(eng, spec, kw):
    """every batch chunk in a pass of its own: row 3's last frame then crosses a pass boundary in the spare row"""
    pro, codes, seeds, _, rag, spans, _ = _chunked(eng, spec)
    got, sp = _cat(eng.decode_chunked(pro, codes, seeds, CHUNK, HALO, frame_lens=FRAMES, **kw))
    assert sp == spans and torch.equal(got, rag)


def test_decode_chunked_device_lengths(eng, spec):
    """a device frame_lens tensor (read back once) gives the same bits as the host list"""
    pro, codes, seeds, _, rag, _, _ = _chunked(eng, spec)
    got, _ = _cat(eng.decode_chunked(pro, codes, seeds, CHUNK, HALO, frame_lens=pro["frame_lens"]))
    assert torch.equal(got, rag)


def test_full_length_rows_equal_the_uniform_decode_chunked(eng, spec):
    S, dev = spec, eng.device
    g = torch.Generator().manual_seed(5)
    h = torch.randn(B, T, S.d_txt, generator=g).to(torch.bfloat16).float()
    codes = (torch.randn(B, S.L_s, S.code_dim, generator=g) * 0.3).to(dev)
    dur = torch.tensor([_split(7)] * B, dtype=torch.int32)
    pro = eng.predict_prosody(_h_act(eng, h), codes, dur)
    uni, su = _cat(eng.decode_chunked(pro, codes, [1, 2, 3, 4], CHUNK, HALO), S.frame40 * 7)
    rag, sr = _cat(eng.decode_chunked(pro, codes, [1, 2, 3, 4], CHUNK, HALO, frame_lens=[7] * B), S.frame40 * 7)
    assert su == sr and torch.equal(rag, uni)


def test_synth_stream_chunked_ragged_equals_the_decode(eng, spec):
    """synth_stream(chunked_halo=1, ragged_frames=True) is the front, then decode_chunked on the predicted counts"""
    S = spec
    tok, ref, eps, rl, dur = _synth_inputs(S)
    chunk_s = CHUNK * S.frame40 / S.sr
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, durations=dur, seeds=[3, 4, 5, 6], text_lens=TEXT_LENS, ref_lens=rl)
    width = S.frame40 * max(FRAMES)
    got, spans = _cat(eng.synth_stream(tok, ref, chunk_s=chunk_s, chunked_halo=HALO, ragged_frames=True, **kw), width)
    assert eng.frame_lens.cpu().tolist() == FRAMES
    _, _, codes, pro, seeds = eng._front(tok, ref, STEPS, CFG, eps, dur, [3, 4, 5, 6], None, None, None, TEXT_LENS, rl,
                                         True)
    want, sw = _cat(eng.decode_chunked(pro, codes, seeds, CHUNK, HALO, frame_lens=FRAMES), width)
    assert spans == sw and torch.equal(got, want)
    for b, n in enumerate(FRAMES):
        assert bool((got[b, S.frame40 * n:] == 0).all())
