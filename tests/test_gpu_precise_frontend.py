"""The precise reference-prompt front end (StyleTTSZS(precise_frontend=True)) vs float64 restatements and the fp32
oracle, and FREE-RUNNING end-to-end parity: synth() against oracle.synth() from the same reference wav with no
prompt code teacher-forced.

Stated tolerances.
  log-mel (stzs_stft_logmel, csrc/stftmel.hip) vs an fp64 restatement (torch.stft, HTK filterbank and log in float64):
    L1 <= 4 x and max-abs <= max(4 x, 1e-5) of the fp32 oracle's own distance to the same fp64 reference on the same
    input -- the factor covers another FFT factorisation / summation order and the GPU logf; cells whose fp64 mel power
    is within 1e-9 relative of the 1e-5 clamp (a kink of the derivative, not of the value) are held to atol 1e-5.
  pre-quantiser features z vs an fp64 restatement of oracle.prompt_features: rel-L2 <= Z_REL_L2 (twice the measured
    value, one significant digit) and max-abs <= 1e-4 (the error at which the code guard below still leaves >= 98 % of
    the codes checkable).
  discrete codes: equal to the oracle's on every CLEAR code -- with delta = max|z_gpu - z_oracle|, a code is clear when
    for every k != best  d_k - d_best > 2 delta (|z - c_k|_1 + |z - c_best|_1) + 2 dg delta^2 + 1e-6  (the first-order
    bound on how far delta moves a distance difference; 1e-6 for the fp32 distance sums) -- and at most 2 % unclear.
  free running (precise + precise_frontend): prompt codes and durations equal to the oracle's, log-mel L1 of the
    waveform <= 1e-3 (the north-star bound)."""
import math

import pytest
import torch
import torch.nn.functional as F

from refops import rel_err

pytestmark = pytest.mark.gpu

# measured on MI355X (the prints of test_precise_prompt_features): rel-L2 vs fp64 7.3e-6 (tiny) / 6.1e-6 (v0), max-abs
# 6.1e-6 / 5.1e-6 -- the split-operand convs' dropped lo * lo products; the fp32 oracle itself is 1.5e-7 / 2.4e-7 off.
# Twice the larger one, rounded up to one significant digit:
Z_REL_L2 = 2e-5


@pytest.fixture(scope="module")
def tiny_pf(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    return StyleTTSZS(tiny, tiny_params, device=gpu_device, precise_frontend=True), tiny, tiny_params


@pytest.fixture(scope="module")
def v0_pf(gpu_device):
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.spec import SPEC_V0
    torch.set_num_threads(16)
    P = init_params(SPEC_V0, seed=0)
    return StyleTTSZS(SPEC_V0, P, device=gpu_device, precise=True, precise_frontend=True), SPEC_V0, P


def _pick(spec, tiny_pf, v0_pf):
    return tiny_pf if spec == "tiny" else v0_pf


def _fb64(n_mels, n_fft, sr):
    """oracle.htk_mel_filterbank kept in float64"""
    to_mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    to_hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    top = to_mel(sr / 2.0)
    edges = [to_hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)]
    nb = n_fft // 2 + 1
    freqs = torch.linspace(0.0, sr / 2.0, nb, dtype=torch.float64)
    fb = torch.zeros(n_mels, nb, dtype=torch.float64)
    for m in range(n_mels):
        lo, ce, hi = edges[m], edges[m + 1], edges[m + 2]
        fb[m] = torch.clamp(torch.minimum((freqs - lo) / max(ce - lo, 1e-9), (hi - freqs) / max(hi - ce, 1e-9)), min=0.0)
    return fb


def _melpow64(wav, S):
    X = torch.stft(wav.double(), S.mel_nfft, hop_length=S.hop, win_length=S.mel_win,
                   window=torch.hann_window(S.mel_win, dtype=torch.float64), center=True, return_complex=True)
    return _fb64(S.n_mels, S.mel_nfft, S.sr) @ X.abs().square()  # [B, n_mels, F]


def _logmel64(wav, S):
    return torch.log(torch.clamp(_melpow64(wav, S), min=1e-5))


def _z64(P, S, ref):
    """oracle.prompt_features in float64"""
    D = lambda n: P[n].double()
    x = F.leaky_relu(F.conv1d(_logmel64(ref, S), D("pe.conv0.w"), D("pe.conv0.b"), padding=2), 0.2)
    x = F.leaky_relu(F.conv1d(x, D("pe.conv1.w"), D("pe.conv1.b"), padding=2), 0.2)
    x = F.adaptive_avg_pool1d(x, S.L_s).transpose(1, 2)
    return F.linear(x, D("pe.proj.w"), D("pe.proj.b"))


def _wav(B, N):
    wav = torch.randn(B, N, generator=torch.Generator().manual_seed(5)) * 0.1
    if N == 7501:  # silent frames and a level ramp from 0: cells on and around the 1e-5 clamp
        wav[0, 2000:5000] = 0
        wav[1] *= torch.linspace(0, 3, N)
    return wav


_REF64 = {}


def _logmel_case(spec, S, B, N):
    """(wav, fp64 mel power, fp64 log-mel, fp32 oracle log-mel) of a case, computed once"""
    from oracle import stzs_ref as R
    key = (spec, B, N)
    if key not in _REF64:
        wav = _wav(B, N)
        pw = _melpow64(wav, S)
        _REF64[key] = (wav, pw, torch.log(torch.clamp(pw, min=1e-5)), R.log_mel(wav, S))
    return _REF64[key]


def _gpu_logmel(eng, S, wav):
    mel = eng.log_mel(wav.to(eng.device).contiguous())
    assert mel.t.dtype == torch.float32
    return mel.t[:, :, :S.n_mels].cpu().transpose(1, 2)  # [B, n_mels, F] as the oracle


@pytest.mark.parametrize("spec,B,N", [("tiny", 2, 1025), ("tiny", 2, 7501), ("tiny", 3, 30001), ("v0", 2, 7501)])
def test_stft_logmel_vs_fp64(tiny_pf, v0_pf, spec, B, N):
    eng, S, _ = _pick(spec, tiny_pf, v0_pf)
    wav, pw, ref, orc = _logmel_case(spec, S, B, N)
    got = _gpu_logmel(eng, S, wav)
    assert got.shape == ref.shape == (B, S.n_mels, N // S.hop + 1)
    near = (pw - 1e-5).abs() <= 1e-9 * 1e-5  # on the clamp's kink: absolute tolerance only
    far = ~near
    eg, eo = (got.double() - ref).abs(), (orc.double() - ref).abs()
    l1_g, l1_o = eg[far].mean().item(), eo[far].mean().item()
    mx_g, mx_o = eg[far].max().item(), eo[far].max().item()
    clamped = (pw <= 1e-5).double().mean().item()
    print(f"stft_logmel {spec} B {B} N {N}: L1 {l1_g:.3e} (oracle {l1_o:.3e}) max {mx_g:.3e} (oracle {mx_o:.3e}) "
          f"clamped {clamped:.3f} near-kink {int(near.sum())}")
    assert torch.isfinite(got).all()
    assert bool((eg[near] <= 1e-5).all())
    assert l1_g <= 4 * l1_o
    assert mx_g <= max(4 * mx_o, 1e-5)


def test_stft_logmel_batch_invariant(tiny_pf):
    eng, S, _ = tiny_pf
    wav = _logmel_case("tiny", S, 3, 30001)[0]
    full = _gpu_logmel(eng, S, wav)
    for r in (0, 2):
        one = _gpu_logmel(eng, S, wav[r:r + 1])
        assert torch.equal(one[0], full[r]), r


# n_fft, win, hop, N, n_mels: the transform sizes the engines never use -- the smallest (one 32-word block per plane, two
# radix-4 stages + the radix-2 one), log2(n_fft / 2) even and odd (1024, 4096: the radix-2 tail stage; 4096 also the
# largest LDS footprint and two butterflies per thread), win == n_fft and win < n_fft, N not a multiple of hop
FFT_SIZES = [(64, 64, 16, 100, 4), (128, 100, 32, 333, 6), (512, 512, 128, 2000, 16), (1024, 600, 150, 3001, 16),
             (4096, 2400, 600, 9001, 16)]


@pytest.mark.parametrize("n_fft,win,hop,N,n_mels", FFT_SIZES)
def test_stft_logmel_fft_sizes(gpu_device, n_fft, win, hop, N, n_mels):
    """stzs_stft_logmel through the C ABI at other transform sizes, against the float64 evaluation of the same inputs
    (the fp32 window and filterbank taken as given); yardstick as above: a plain torch fp32 evaluation's own distance,
    L1 <= 4 x, max-abs <= max(4 x, 1e-5).  The bf16 output is the fp32 one rounded to nearest even, exactly."""
    from stzs import _lib as L_
    from stzs.frontend import mel_filterbank
    from stzs.weights import stft_twiddles
    lib = L_.load()
    B, Fr = 2, N // hop + 1
    wav = torch.randn(B, N, generator=torch.Generator().manual_seed(n_fft)) * 0.1
    window, fb = torch.hann_window(win), mel_filterbank(n_mels, n_fft, 24000).contiguous()
    rng = torch.zeros(n_mels, 2, dtype=torch.int32)
    for m in range(n_mels):
        nz = (fb[m] > 0).nonzero()
        assert len(nz) >= 2, "every filter spans several bins"
        rng[m, 0], rng[m, 1] = int(nz[0]), int(nz[-1]) + 1

    def ref(dt):
        X = torch.stft(wav.to(dt), n_fft, hop_length=hop, win_length=win, window=window.to(dt), center=True,
                       return_complex=True)
        return torch.log(torch.clamp(fb.to(dt) @ (X.real ** 2 + X.imag ** 2), min=1e-5)).transpose(1, 2)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    dev = [t.to(gpu_device) for t in (wav, window, stft_twiddles(n_fft), fb, rng)]
    outs = {}
    for dt, code in ((torch.float32, L_.F32), (torch.bfloat16, L_.BF16)):
        y = torch.full((B, Fr, n_mels + 3), 7.0, dtype=dt, device=gpu_device)  # a row pitch wider than n_mels
        a = L_.StftMelArgs()
        a.wav, a.window, a.twiddle, a.fb, a.ranges = (t.data_ptr() for t in dev)
        a.y, a.ldw, a.ldy, a.bsy = y.data_ptr(), N, n_mels + 3, Fr * (n_mels + 3)
        a.B, a.N, a.F, a.n_fft, a.win, a.hop, a.n_mels, a.out_dtype = B, N, Fr, n_fft, win, hop, n_mels, code
        L_.check(lib.stzs_stft_logmel(a, None), "stft_logmel")
        torch.cuda.synchronize()
        assert bool((y[:, :, n_mels:] == 7.0).all()), "columns past n_mels written"
        outs[dt] = y[:, :, :n_mels].cpu()
    eg, eo = (outs[torch.float32].double() - r64).abs(), (r32.double() - r64).abs()
    print(f"stft_logmel n_fft {n_fft} win {win} hop {hop} N {N}: L1 {eg.mean().item():.3e} (torch fp32 "
          f"{eo.mean().item():.3e}) max {eg.max().item():.3e} (torch fp32 {eo.max().item():.3e})")
    assert eg.mean().item() <= 4 * eo.mean().item()
    assert eg.max().item() <= max(4 * eo.max().item(), 1e-5)
    assert torch.equal(outs[torch.bfloat16], outs[torch.float32].to(torch.bfloat16))


def _prompt_ref(S):
    return torch.randn(2, 3 * S.sr, generator=torch.Generator().manual_seed(11)) * 0.1


@pytest.mark.parametrize("spec", ["tiny", "v0"])
def test_precise_prompt_features(tiny_pf, v0_pf, spec):
    from oracle import stzs_ref as R
    eng, S, P = _pick(spec, tiny_pf, v0_pf)
    ref = _prompt_ref(S)
    z64 = _z64(P, S, ref)
    z = eng.prompt_features(ref.to(eng.device)).cpu().double()
    zo = R.prompt_features(P, S, ref).double()
    e, mx = rel_err(z, z64), (z - z64).abs().max().item()
    print(f"precise prompt features {spec}: rel-L2 {e:.3e} max-abs {mx:.3e} vs fp64 "
          f"(fp32 oracle: {rel_err(zo, z64):.3e} / {(zo - z64).abs().max().item():.3e})")
    assert e <= Z_REL_L2
    assert mx <= 1e-4


def _clear_codes(P, S, z, idx, delta):
    """[R, G] bool: the oracle's decision for z (fp32 [B, L, code]) cannot be moved by an error of delta per value"""
    cb = P["pe.vq"].double()  # [G, K, dg]
    G, K, dg = cb.shape
    diff = z.double().reshape(-1, G, 1, dg) - cb[None]
    d, l1 = diff.square().sum(-1), diff.abs().sum(-1)  # [R, G, K]
    best = idx.reshape(-1, G, 1).long()
    gap = d - d.gather(2, best)
    thr = 2 * delta * (l1 + l1.gather(2, best)) + 2 * dg * delta * delta + 1e-6
    ok = gap > thr
    ok.scatter_(2, best, True)  # k = best itself
    return ok.all(-1)


@pytest.mark.parametrize("spec,inputs", [("tiny", "seed11"), ("v0", "seed11"), ("v0", "configs1")])
def test_precise_prompt_codes(tiny_pf, v0_pf, spec, inputs):
    import bench
    from oracle import stzs_ref as R
    eng, S, P = _pick(spec, tiny_pf, v0_pf)
    ref = _prompt_ref(S) if inputs == "seed11" else bench.make_inputs(S, 1, 1000)[1]
    zo = R.prompt_features(P, S, ref)
    idx_o = R.quantize_codes(P, S, zo)[0]
    z = eng.prompt_features(ref.to(eng.device)).cpu()
    got = eng.prompt_encode(ref.to(eng.device)).cpu()
    idx = eng.prompt_idx.cpu()
    delta = (z - zo).abs().max().item()
    clear = _clear_codes(P, S, zo, idx_o, delta).reshape(idx_o.shape)
    unclear = 1.0 - clear.double().mean().item()
    agree = idx == idx_o
    print(f"precise prompt codes {spec} {inputs}: delta {delta:.3e} unclear {int((~clear).sum())} of {clear.numel()} "
          f"({unclear:.4f}) mismatches {int((~agree).sum())}")
    assert bool(agree[clear].all())
    assert unclear <= 0.02
    assert torch.equal(got, R.lookup_codes(P, S, idx))


def _logmel_l1(a, b, S):
    from oracle import stzs_ref as R
    return (R.log_mel(a, S) - R.log_mel(b, S)).abs().mean().item()


def _parity(out, o, S, what):
    m_w = _logmel_l1(out["wav"].cpu(), o["wav"], S)
    print(f"free-running {what}: prompt codes equal {torch.equal(out['prompt_idx'].cpu(), o['prompt_idx'])} "
          f"codes {rel_err(out['codes'].cpu(), o['codes']):.2e} F0 {rel_err(out['F0'].cpu(), o['F0']):.2e} "
          f"wav {rel_err(out['wav'].cpu(), o['wav']):.2e} log-mel L1 {m_w:.3e}")
    assert torch.equal(out["prompt_idx"].cpu(), o["prompt_idx"])
    assert torch.equal(out["dur"].cpu(), o["dur"].to(out["dur"].dtype))
    assert m_w <= 1e-3


def test_free_running_parity_configs1(v0_pf):
    """configs[1] (batch 1, 10 steps, CFG 5) with NOTHING teacher-forced: the oracle quantises its own prompt features.
    (reference seed 1004: the oracle's smallest code margin is 6.8e-5, every code clear at delta 1e-5)"""
    import bench
    from oracle import stzs_ref as R
    eng, S, P = v0_pf
    tok, ref, eps, dur = bench.make_inputs(S, 1, seed=1004)
    steps, seeds = 10, [7]
    out = eng.synth(tok, ref, steps=steps, cfg_scale=5.0, noise=eps, durations=dur, seeds=seeds)
    eng.check_status()
    o = R.synth(P, S, tok, ref, steps, 5.0, eps, dur, seeds=seeds)
    _parity(out, o, S, "configs1")


def test_free_running_parity_batch4(v0_pf):
    """four utterances, 2 steps, CFG 5, nothing teacher-forced (reference wavs with oracle code margins >= 7.1e-5);
    row 2 alone gives the same bits."""
    import bench
    from oracle import stzs_ref as R
    eng, S, P = v0_pf
    ref = torch.cat([bench.make_inputs(S, 1, s)[1] for s in (1010, 1020, 1041, 1054)], 0)
    tok, _, eps, dur, seeds = bench.rank_inputs(S, 4, 0)
    out = eng.synth(tok, ref, steps=2, cfg_scale=5.0, noise=eps, durations=dur, seeds=seeds)
    eng.check_status()
    keep = {k: out[k].detach().clone().cpu() for k in ("prompt_idx", "wav")}
    o = R.synth(P, S, tok, ref, 2, 5.0, eps, dur, seeds=seeds)
    _parity(out, o, S, "batch4")
    o1 = eng.synth(tok[2:3], ref[2:3], steps=2, cfg_scale=5.0, noise=eps[2:3], durations=dur[2:3], seeds=seeds[2:3])
    for k in ("prompt_idx", "wav"):
        assert torch.equal(o1[k].cpu(), keep[k][2:3]), k


def test_precise_prompt_graph_replay(gpu_device, tiny, tiny_params):
    """prompt_encode of the precise front end captured in one graph (single stream) and replayed on new reference
    samples in the same buffer: the eager call's bits."""
    from stzs.engine import StyleTTSZS
    S = tiny
    eng = StyleTTSZS(S, tiny_params, device=gpu_device, precise_frontend=True)
    assert not eng.branch_streams
    g = torch.Generator().manual_seed(21)
    ref0, ref1 = (torch.randn(2, S.sr, generator=g) * 0.1 for _ in range(2))
    buf = ref0.to(gpu_device)
    graph, out = eng.capture(lambda: eng.prompt_encode(buf))
    idx = eng.prompt_idx
    buf.copy_(ref1.to(gpu_device))
    got = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got.append((out.clone(), idx.clone()))
    eager = StyleTTSZS(S, tiny_params, device=gpu_device, precise_frontend=True)
    want = eager.prompt_encode(ref1.to(gpu_device)).clone()
    want_idx = eager.prompt_idx.clone()
    for q, i in got:
        assert torch.equal(q, want) and torch.equal(i, want_idx)
    eager.prompt_encode(ref0.to(gpu_device))
    assert not torch.equal(want_idx, eager.prompt_idx)  # (the two references give different codes)


def _launch_names(eng, fn):
    names, orig = [], eng._call

    def rec(f, arg, what, **kw):
        names.append(what)
        return orig(f, arg, what, **kw)
    eng._call = rec
    try:
        fn()
    finally:
        del eng._call
    return names


def test_default_front_end_unchanged(gpu_device, tiny, tiny_params, tiny_pf):
    """without the flag -- bf16 default and precise=True alike -- the front end is the bf16 one: frames, DFT GEMM and
    log-mel launches, a bf16 log-mel; with it, the one fused launch and fp32 rows."""
    from stzs.engine import StyleTTSZS
    ref = (torch.randn(1, tiny.sr, generator=torch.Generator().manual_seed(3)) * 0.1).to(gpu_device)
    for kw in (dict(), dict(precise=True)):
        eng = StyleTTSZS(tiny, tiny_params, device=gpu_device, **kw)
        assert not eng.precise_frontend and not eng.W.precise_frontend
        names = _launch_names(eng, lambda: eng.prompt_encode(ref))
        assert "stft_frames" in names and "fe.dft" in names and "log_mel" in names and "stft_logmel" not in names, names
        assert eng._bufs[("fe.mel", torch.bfloat16)][2].dtype == torch.bfloat16
        assert ("fe.mel", torch.float32) not in eng._bufs
        assert eng.W.pe_conv0.wx3 is None
    eng = tiny_pf[0]
    names = _launch_names(eng, lambda: eng.prompt_encode(ref))
    assert names == ["stft_logmel", "pe.conv0", "pe.conv1", "pool_rows", "pe.proj", "code_quantize"], names
    assert ("fe.mel", torch.bfloat16) not in eng._bufs
