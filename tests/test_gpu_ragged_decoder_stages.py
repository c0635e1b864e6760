"""The ragged decoder through the engine: decode(frame_lens=...) and synth(ragged_frames=True) on the
default engine, on the smallest spec that passes _check_ragged_decoder -- SPEC_TINY with dec_out 128 and gen_ch
(256, 128): register-direct Snake convs in their multi-chunk (stage 0) and single-chunk (stage 1) forms, the
polyphase ConvTranspose with a residual (stage 0) and with the fused noise conv (stage 1), conv_post on the narrow form.

B = 4 rows with forced durations of [7, 1, 3, 6] frames: 14 / 2 / 6 / 12 decoder output rows, 140 / 20 / 60 / 120
stage-0 rows (across the 64-row statistics chunk and the 128-row tile), 841 / 121 / 361 / 721 stage-1 rows and iSTFT
frames.  Row b of the ragged batch must be, bit for bit, what the same engine computes for that row alone at T40 = T_b:
every traced stage's valid rows and wav[b, :600 T_b]; the waveform tail is exact zeros."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T = 4, 12
FRAMES = [7, 1, 3, 6]
TEXT_LENS = [12, 5, 9, 3]
STEPS, CFG = 2, 5.0


def _split(n, T=T):
    return [n // T + (1 if t < n % T else 0) for t in range(T)]


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


def _inputs(S, seed=99):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, T, S.d_txt, generator=g).to(torch.bfloat16).float()
    codes = torch.randn(B, S.L_s, S.code_dim, generator=g) * 0.3
    return h, codes


def _h_act(eng, h):
    from stzs.engine import Act
    t = torch.zeros(*h.shape, dtype=eng.adt, device=eng.device)
    t.copy_(h.to(eng.adt))
    return Act(t)


def _rows_of(S, n):
    """valid rows of every traced stage for a row of n frames"""
    r0, r1 = S.up_rates
    return dict(gen_in=2 * n, har=2 * n * S.hop // S.istft_hop + 1, mrf_in0=2 * n * r0, mrf_out0=2 * n * r0,
                mrf_in1=2 * n * r0 * r1 + 1, mrf_out1=2 * n * r0 * r1 + 1, post=2 * n * r0 * r1 + 1)


def _host_trace(tr):
    """host copies of the traced activations (the engine's buffers are reused by the next call)"""
    return {k: v.t[:, :, v.c0:v.c0 + v.C].cpu().clone() for k, v in tr.items()}


def _decode(eng, S, h, codes, dur, seeds, ragged):
    """prosody + decode with the trace -> (wav, host trace, frame_lens | None)"""
    dev = eng.device
    pro = eng.predict_prosody(_h_act(eng, h), codes.to(dev), dur, ragged_frames=ragged)
    tr = {}
    if ragged:
        wav = eng.decode(pro, codes.to(dev), seeds, frame_lens=pro["frame_lens"], trace=tr)
    else:
        wav = eng.decode(pro, codes.to(dev), seeds, trace=tr)
    return wav.cpu().clone(), _host_trace(tr), (pro["frame_lens"].cpu().clone() if ragged else None)


_runs = {}


def _forced(eng, S):
    if "forced" not in _runs:
        h, codes = _inputs(S)
        dur = torch.tensor([_split(n) for n in FRAMES], dtype=torch.int32)
        rag = _decode(eng, S, h, codes, dur, [10, 11, 12, 13], True)
        solos = [_decode(eng, S, h[b:b + 1], codes[b:b + 1], dur[b:b + 1], [10 + b], False) for b in range(B)]
        assert eng.check_status() == 0
        _runs["forced"] = (h, codes, dur, rag, solos)
    return _runs["forced"]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _check(S, rag, solos, frames):
    wav, tr, fl = rag
    n40 = S.frame40
    assert fl.tolist() == frames and wav.shape == (len(frames), n40 * max(frames))
    assert bool(torch.isfinite(wav).all())
    for b, n in enumerate(frames):
        w1, t1, _ = solos[b]
        assert w1.shape == (1, n40 * n)
        for k, rows in _rows_of(S, n).items():
            assert t1[k].shape[1] == rows, (k, t1[k].shape, rows)
            assert torch.equal(_bits(tr[k][b, :rows]), _bits(t1[k][0])), f"row {b} ({n} frames): stage {k} differs"
            assert bool(torch.isfinite(tr[k][b].float()).all()), f"row {b}: stage {k} has a non-finite tail"
        assert torch.equal(wav[b, :n40 * n], w1[0]), f"row {b} ({n} frames): waveform differs from its solo decode"
        assert bool((wav[b, n40 * n:] == 0).all()), f"row {b}: waveform tail is not exact zeros"
        nh = _rows_of(S, n)["har"]
        assert bool((tr["har"][b, nh:] == 0).all()), f"row {b}: har rows past its own frames are not zeros"


def test_decode_rows_match_solo(eng, spec):
    _, _, _, rag, solos = _forced(eng, spec)
    _check(spec, rag, solos, FRAMES)


def test_full_length_rows_equal_the_plain_decode(eng, spec):
    """every row at the padded width: the ragged decode is the plain decode, bit for bit"""
    S, dev = spec, eng.device
    h, codes = _inputs(S, 5)
    dur = torch.tensor([_split(7)] * B, dtype=torch.int32)
    pro = eng.predict_prosody(_h_act(eng, h), codes.to(dev), dur)
    plain = eng.decode(pro, codes.to(dev), [1, 2, 3, 4]).clone()
    fl = torch.full((B,), 7, dtype=torch.int32, device=dev)
    rag = eng.decode(pro, codes.to(dev), [1, 2, 3, 4], frame_lens=fl)
    assert torch.equal(rag, plain)


def test_fork_rows_match_solo(gpu_device, spec, params, eng):
    """with the decoder pre-blocks || harmonic source fork on (side stream), the rows still equal the solo run"""
    from stzs.engine import StyleTTSZS
    h, codes, dur, _, solos = _forced(eng, spec)
    e2 = StyleTTSZS(spec, params, device=gpu_device, branch_streams={"src"})
    rag = _decode(e2, spec, h, codes, dur, [10, 11, 12, 13], True)
    assert e2.check_status() == 0
    _check(spec, rag, solos, FRAMES)


def test_ragged_decode_captures(gpu_device, spec, params):
    """the ragged decode makes no host sync: captured into a graph, its replay equals the eager result"""
    from stzs.engine import StyleTTSZS
    S = spec
    e2 = StyleTTSZS(S, params, device=gpu_device)  # (its own buffer cache: a capture pins its shapes)
    h, codes = _inputs(S)
    dur = torch.tensor([_split(n) for n in FRAMES], dtype=torch.int32)
    cd = codes.to(gpu_device)
    pro = e2.predict_prosody(_h_act(e2, h), cd, dur, ragged_frames=True)
    seeds = torch.tensor([10, 11, 12, 13], dtype=torch.int32, device=gpu_device)

    def run():
        return e2.decode(pro, cd, seeds, frame_lens=pro["frame_lens"])

    eager = run().clone()
    graph, out = e2.capture(run)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert graph.check() == 0
    assert torch.equal(out, eager)


def test_synth_ragged_frames_matches_solo_synth(eng, spec):
    """synth(ragged_frames=True) end to end, predicted durations, ragged text and ragged references at the same time:
    each row's samples equal its solo synth(), the tail is zeros"""
    S, dev = spec, eng.device
    g = torch.Generator().manual_seed(31)
    tok = torch.randint(1, S.n_symbols, (B, T), generator=g)
    N = S.sr // 2
    ref = torch.randn(B, N, generator=g) * 0.1
    eps = torch.randn(B, S.L_s, S.code_dim, generator=g)
    rl = [N, 7 * N // 10 + 1, N, S.mel_nfft // 2 + 1]
    wav, fl = eng.synth(tok, ref, steps=STEPS, cfg_scale=CFG, noise=eps, seeds=[3, 4, 5, 6], text_lens=TEXT_LENS,
                        ref_lens=rl, ragged_frames=True)
    wav, fl = wav.cpu().clone(), fl.cpu().tolist()
    print("predicted frame counts", fl)
    assert wav.shape == (B, S.frame40 * max(fl))
    for b, n in enumerate(TEXT_LENS):
        one = eng.synth(tok[b:b + 1, :n], ref[b:b + 1, :rl[b]], steps=STEPS, cfg_scale=CFG, noise=eps[b:b + 1],
                        seeds=[3 + b])["wav"].cpu()
        assert one.shape == (1, S.frame40 * fl[b]), (one.shape, fl[b])
        assert torch.equal(wav[b, :one.shape[1]], one[0]), f"row {b} differs from its solo synth()"
        assert bool((wav[b, one.shape[1]:] == 0).all())
