"""CPU self-checks of the back-end references in tests/refops.py (used by tests/test_gpu_backend.py): source_ref against
the oracle's fp32 and fp64 sources, istft_ref against fp64 torch.istft, the span and alignment restatements, the
duration cases' tie shares -- and numpy emulations of the kernels' fp32 arithmetic: the honest one inside every bound
of the GPU file, each emulation with one planted defect outside it by a wide margin."""
import math

import numpy as np
import pytest
import torch

from refops import (DUR_NBINS, DUR_ROWS, E_RR, ISTFT_GEOMS, SHIPPED, align_ref, dur_logits, dur_tie_width, durations_ref,
                    f0_case, istft_bound, istft_halo, istft_ref, istft_span_ref, merge_weights, post_case, reflect_index,
                    source_bound, source_ref, source_theta32, uniforms24)

# ---- the references against independent restatements ---------------------------------------------------------------

class _Spec:
    """the fields oracle.harmonic_source reads, at the shipped geometry"""
    harmonic_num, sr, hop, n_fft, istft_hop = 8, 24000, 300, 20, 5
    sine_amp, noise_std, voiced_threshold = 0.1, 0.003, 10.0


def _oracle_bins(F0, seeds, mw):
    from oracle.stzs_ref import source_features
    P = {"gen.src_merge.w": torch.from_numpy(mw[None, :-1].copy()), "gen.src_merge.b": torch.from_numpy(mw[-1:].copy())}
    X, src = source_features(P, _Spec, F0, seeds)
    return X.transpose(1, 2).double().numpy(), src.double().numpy()


def test_source_ref_vs_oracle():
    """shipped geometry: within 1e-5 of the maximum of the fp32 oracle; against the fp64 oracle the distance is the
    fp32 in-frame phase the reference shares with the kernel (4e-6 cycles at 60 cycles, here up to 135
    cycles at 900 Hz x 9 -> 1.6e-5 cycles -> 2 pi 1.6e-5 x 0.1 x sum|w| per sample): 1e-4 of the maximum"""
    B, T80, nh = 2, 13, 9
    f0 = f0_case(B, T80, SHIPPED["voiced_thr"], "oracle")
    mw, seeds = merge_weights(nh), [11, 0x80000000]
    r = source_ref(f0, seeds, mw, nh=nh, **SHIPPED)
    b32, x32 = _oracle_bins(torch.from_numpy(f0), seeds, mw)
    b64, x64 = _oracle_bins(torch.from_numpy(f0).double(), seeds, mw)
    top = np.abs(b64).max()
    e32, e64 = np.abs(r["bins"] - b32).max() / top, np.abs(r["bins"] - b64).max() / top
    print(f"source_ref vs oracle: fp32 {e32:.2e}, fp64 {e64:.2e} of the maximum; samples {np.abs(r['x'] - x32).max():.2e}")
    assert e32 <= 1e-5 and e64 <= 1e-4
    assert r["bins"].shape == (B, T80 * 300 // 5 + 1, 22)


@pytest.mark.parametrize("n_fft,hop_s", sorted(ISTFT_GEOMS))
def test_istft_ref_vs_torch(n_fft, hop_s):
    """fp64 torch.istft on the same spectrum at 1e-12 relative, for every geometry of the GPU file; the envelope of every
    emitted sample is above 1e-3 (the non-zero-overlap-add condition with room)"""
    nb, halo = n_fft // 2 + 1, ISTFT_GEOMS[(n_fft, hop_s)]
    assert istft_halo(n_fft, hop_s) == halo
    for Tf in (2, 3, halo + 1, 256 - halo + 1, 601):
        p = post_case(2, Tf, n_fft, "small", (n_fft, hop_s, Tf))
        wav, S, env = istft_ref(p, n_fft, hop_s)
        pd = torch.from_numpy(p).double()
        spec = torch.exp(pd[:, :, :nb]) * torch.exp(1j * torch.sin(pd[:, :, nb:2 * nb]))
        ref = torch.istft(spec.transpose(1, 2), n_fft, hop_length=hop_s, win_length=n_fft,
                          window=torch.hann_window(n_fft, dtype=torch.float64)).numpy()
        assert wav.shape == ref.shape == (2, (Tf - 1) * hop_s)
        assert env > 1e-3
        assert np.abs(wav - ref).max() <= 1e-12 * np.abs(ref).max()
        assert (np.abs(wav) <= S * (1 + 1e-12)).all()


def test_span_ref_tiles():
    for (n_fft, hop_s), halo in ISTFT_GEOMS.items():
        for chunks in ([1] * 9, [2, 7], [5, 3, 1], [9]):
            f0 = nxt = 0
            for i, Fc in enumerate(chunks):
                n0, n1, h = istft_span_ref(f0, Fc, i == len(chunks) - 1, n_fft, hop_s)
                assert h == halo and n0 == nxt and n1 >= n0
                f0, nxt = f0 + Fc, n1
            assert nxt == 8 * hop_s


def test_align_ref():
    d = np.array([[0, 2, 0, 3, 0], [1, 1, 1, 0, 0], [0, 0, 0, 0, 0]], np.int32)
    idx, tot = align_ref(d, 6)
    assert idx.tolist() == [[1, 1, 3, 3, 3, -1], [0, 1, 2, -1, -1, -1], [-1] * 6] and tot.tolist() == [5, 3, 0]
    assert align_ref(d, 2)[0].tolist() == [[1, 1], [0, 1], [-1, -1]]


@pytest.mark.parametrize("nbins", DUR_NBINS)
def test_duration_cases_have_few_ties(nbins):
    """the GPU file's duration inputs: under 1 % of the fp64 sums lie within the tie width of a half-integer (so the
    share condition can only fail through the kernel), and +-100 logits give exactly the clamp"""
    near = total = 0
    for rows in DUR_ROWS:
        _, s, dist = durations_ref(dur_logits(rows, nbins))
        near, total = near + int((dist <= dur_tie_width(nbins)).sum()), total + dist.size
    assert near < 0.01 * total, (near, total)
    d, s, _ = durations_ref(np.stack([np.full((3, nbins), 100.0), np.full((3, nbins), -100.0)]).astype(np.float32))
    assert (d[0] == nbins).all() and (d[1] == 1).all()


# ---- emulations of the kernels' arithmetic ----------------------------------------------------------------------------

def emu_source(f0, seeds, mw, *, hop, n_fft, hop_s, nh, sr, sine_amp, noise_std, voiced_thr, mut=None):
    """csrc/source.hip in numpy fp32: every padded sample from its reflected index, the sine and the Box-Muller cosine
    in revolutions on exact arguments (as v_sin / v_cos take them), fp32 merge, tanh, window and DFT sums.
    mut: "counter" (noise counter from the unreflected index), "right" (right reflection 2N - 1 - n), "ge" (F0 >= thr),
    "ph0" (a random initial phase for harmonic 0 too)"""
    f32 = np.float32
    f = np.asarray(f0, f32)
    B, T = f.shape
    N, Tf = T * hop, T * hop // hop_s + 1
    theta, _, keys = source_theta32(f, seeds, hop=hop, nh=nh, sr=sr, first_phase_zero=mut != "ph0")
    p = np.arange((Tf - 1) * hop_s + n_fft)
    n = reflect_index(p, N, n_fft)
    if mut == "right":
        raw = p - n_fft // 2
        n = np.where(raw >= N, 2 * N - 1 - raw, n)
    cnt = ((p - n_fft // 2) if mut == "counter" else n) & 0xFFFFFFFF
    k = n // hop
    x = np.zeros((B, len(p)), f32)
    for b in range(B):
        voiced = (f[b][k] >= f32(voiced_thr)) if mut == "ge" else (f[b][k] > f32(voiced_thr))
        namp = np.where(voiced, f32(noise_std), f32(sine_amp) / f32(3.0)).astype(f32)
        acc = np.zeros(len(p), f32)
        for h in range(nh):
            u1, u2 = uniforms24(keys[b][h], cnt)
            z = np.sqrt(f32(-2.0) * np.log(u1.astype(f32))).astype(f32) * np.cos(2 * math.pi * u2).astype(f32)
            sine = f32(sine_amp) * np.sin(2 * math.pi * theta[b, h][n].astype(np.float64)).astype(f32)
            acc = (acc + f32(mw[h]) * (sine * voiced.astype(f32) + namp * z).astype(f32)).astype(f32)
        x[b] = np.tanh(acc + f32(mw[nh])).astype(f32)
    i = np.arange(n_fft)
    win = (0.5 - 0.5 * np.cos(2 * math.pi * i / n_fft)).astype(f32)
    xi = x[:, np.arange(Tf)[:, None] * hop_s + i[None, :]] * win
    ang = 2 * math.pi * np.outer(i, np.arange(n_fft // 2 + 1)) / n_fft
    return np.concatenate([xi @ np.cos(ang).astype(f32), -(xi @ np.sin(ang).astype(f32))], -1)


def emu_istft(post, n_fft, hop_s, mut=None):
    """csrc/istft.hip in numpy fp32.  mut: "nyquist" (the Nyquist bin's sign (-1)^i dropped), "env" (the envelope
    misses the oldest frame that reaches a sample), "halo" (halo = n_fft / hop_s - 1, floor: the oldest frame's signal
    is not in LDS where hop_s does not divide n_fft, the sum reads zeros)"""
    f32 = np.float32
    p = np.asarray(post, f32)
    B, Tf = p.shape[:2]
    nb, halo = n_fft // 2 + 1, istft_halo(n_fft, hop_s)
    mag, ph = np.exp(p[:, :, :nb]), np.sin(p[:, :, nb:2 * nb].astype(np.float64)).astype(f32)
    re, im = mag * np.cos(ph), mag * np.sin(ph)
    i = np.arange(n_fft)
    ang = 2 * math.pi * np.outer(np.arange(1, nb - 1), i) / n_fft
    sgn = np.ones(n_fft, f32) if mut == "nyquist" else np.where(i % 2, f32(-1), f32(1))
    acc = re[:, :, 1:-1] @ np.cos(ang).astype(f32) - im[:, :, 1:-1] @ np.sin(ang).astype(f32)
    win = (0.5 - 0.5 * np.cos(2 * math.pi * i / n_fft)).astype(f32)
    fr = ((re[:, :, :1] + re[:, :, -1:] * sgn + f32(2) * acc) / f32(n_fft) * win).astype(f32)
    M = (Tf - 1) * hop_s + n_fft
    y, env = np.zeros((B, M), f32), np.zeros(M, f32)
    for t in range(n_fft):
        sl = slice(t, t + Tf * hop_s, hop_s)
        if not (mut == "halo" and t // hop_s > n_fft // hop_s - 1):
            y[:, sl] += fr[:, :, t]
        if not (mut == "env" and t // hop_s == halo):
            env[sl] += win[t] * win[t]
    keep = slice(n_fft // 2, n_fft // 2 + (Tf - 1) * hop_s)
    with np.errstate(divide="ignore", invalid="ignore"):  # (the envelope defect can leave a sample none)
        return y[:, keep] / env[keep]


def source_ratio(got, ref, mw, par):
    bound = source_bound(ref, mw, n_fft=par["n_fft"], sine_amp=par["sine_amp"], noise_std=par["noise_std"])
    return (np.abs(got.astype(np.float64) - ref["bins"]) / bound).max()


SRC_EMU_CASES = [dict(SHIPPED), dict(SHIPPED, hop=240, n_fft=16, hop_s=4, sr=19200.0)]


@pytest.mark.parametrize("par", SRC_EMU_CASES, ids=["20-5-300", "16-4-240"])
def test_source_bound_on_emulations(par):
    """T80 = 13, B = 2 (a row that starts and ends voiced, one unvoiced), nh = 9: the honest emulation inside the fp32
    bound; each defect outside it by more than a factor 20"""
    B, T80, nh = 2, 13, 9
    f0 = f0_case(B, T80, par["voiced_thr"], "emu")
    mw, seeds = merge_weights(nh), [0xFFFFFFFF, 11]
    ref = source_ref(f0, seeds, mw, nh=nh, **par)
    r = {m: source_ratio(emu_source(f0, seeds, mw, nh=nh, mut=m, **par), ref, mw, par)
         for m in (None, "counter", "right", "ge", "ph0")}
    print({k: f"{v:.3g}" for k, v in r.items()})
    assert r[None] <= 1.0
    for m in ("counter", "right", "ge", "ph0"):
        assert r[m] > 20.0, (m, r[m])


@pytest.mark.parametrize("cls", ["small", "mid", "large"])
@pytest.mark.parametrize("n_fft,hop_s", sorted(ISTFT_GEOMS))
def test_istft_bound_on_emulations(n_fft, hop_s, cls):
    """Tf = 601 and Tf = halo + 2 (the shortest row in which a sample has its oldest frame): the honest emulation inside
    the per-sample bound; the Nyquist and envelope defects outside it by more than a factor 100 at Tf = 601 and 10 in
    the short row (every sample of which overlaps the frame with the e^10 bin, which the bound scales with); the floor
    halo likewise wherever hop_s does not divide n_fft (elsewhere it is no defect)"""
    for Tf, far in ((istft_halo(n_fft, hop_s) + 2, 10.0), (601, 100.0)):
        p = post_case(2, Tf, n_fft, cls, (n_fft, hop_s, Tf, cls))
        wav, S, _ = istft_ref(p, n_fft, hop_s)
        bound = istft_bound(S, n_fft, hop_s, cls == "large")
        r = {m: (np.abs(emu_istft(p, n_fft, hop_s, m).astype(np.float64) - wav) / bound).max()
             for m in (None, "nyquist", "env", "halo")}
        assert r[None] <= 1.0, r
        assert r["nyquist"] > far and r["env"] > far, r
        if n_fft % hop_s:
            assert r["halo"] > far, r
        else:
            assert r["halo"] == r[None]


def test_range_reduction_term():
    """the two-constant reduction in fp32 against fp64 x - k 2 pi over the large class: within E_RR of it, and the
    single-constant reduction (the low part removed) beyond E_RR by a factor 100"""
    f32 = np.float32
    g = np.random.default_rng(5)
    x = np.concatenate([g.uniform(-2.0 ** 17, 2.0 ** 17, 200000), [2.0 ** 17 - 0.5, -(2.0 ** 17) + 0.25]]).astype(f32)
    k = np.rint(x * f32(0.159154943091895336)).astype(f32)
    hi, lo = f32(6.28318548202514648), f32(-1.7484555e-7)
    inner = (x.astype(np.float64) - k.astype(np.float64) * np.float64(hi)).astype(f32)       # one fused rounding
    xr = (inner.astype(np.float64) - k.astype(np.float64) * np.float64(lo)).astype(f32)     # and the second
    exact = x.astype(np.float64) - k.astype(np.float64) * 2 * math.pi
    assert np.abs(xr - exact).max() <= E_RR
    assert np.abs(inner - exact).max() > 100 * E_RR
