"""Sample-rate conversion without a GPU: the filter design against its formulas, the quality of the
fp32 tables under the float64 reference (tests/refops_resample.py), the host arithmetic (out_len, span), the public
surface (keyword defaults, the torch operator's fake) and the refusals that need no launch.

Filter quality, measured with the float64 reference on the fp32 tables (a cosine of 8000 samples, 4 K L / M + 50
outputs cut at each end), |y - ideal| in the passband (DC and 0.8 x the lower Nyquist) and |y| in the stopband (1.1 x
and 1.2 x the output Nyquist):

    pair            K    passband   stopband
    24000 -> 48000  69   1.29e-6    -
    24000 -> 16000  103  1.02e-6    1.08e-6
    24000 ->  8000  205  8.91e-7    7.21e-7
    24000 -> 44100  69   2.41e-6    -
    24000 -> 22050  75   1.62e-6    (no tone: see below)
    16000 -> 24000  69   2.04e-6    -
    44100 -> 24000  127  9.72e-7    1.08e-6
    48000 -> 24000  137  6.99e-7    6.81e-7
    24000 -> 24000  1    0          -

The asserted bounds are 4 x the largest value of each column (DESIGN.md §2c's rule: a bound comes from the reference's
own figures, with room for another libm).  24000 -> 22050 has no stopband tone: 1.1 x and 1.2 x its output Nyquist
(12 127 and 13 230 Hz) lie above the INPUT's Nyquist, so no 24 kHz signal holds them -- sampled at 24 kHz they are the
tones at 11 873 and 10 770 Hz, the second inside the band the output keeps.  A stopband tone is therefore measured
where it is below the input Nyquist."""
import inspect
import math

import numpy as np
import pytest
import torch

import refops_resample as R

PASSBAND_MAX, STOPBAND_MAX = 2.41e-6, 1.09e-6  # the table above
K_WANT = {(24000, 48000): 69, (24000, 44100): 69, (16000, 24000): 69, (24000, 16000): 103, (44100, 24000): 127,
          (24000, 8000): 205, (24000, 24000): 1}


@pytest.mark.parametrize("sr_in,sr_out", R.PAIRS, ids=R.PAIR_IDS)
def test_design_matches_its_formulas(sr_in, sr_out):
    from stzs.resample import design
    L, M, W, K, o, h = design(sr_in, sr_out)
    g = math.gcd(sr_in, sr_out)
    assert (L, M) == (sr_out // g, sr_in // g)
    assert o.dtype == np.int32 and o.shape == (L,) and h.dtype == np.float32 and h.shape == (L, (K + 3) // 4 * 4)
    assert not h[:, K:].any()  # the K4 padding columns
    if sr_in == sr_out:
        assert (L, M, W, K) == (1, 1, 0, 1) and o[0] == 0 and h[0, 0] == 1.0
        return
    s = 0.945 * min(1.0, L / M)
    assert W == math.ceil(32 / s) and K == 2 * W + 1
    if (sr_in, sr_out) in K_WANT:
        assert K == K_WANT[(sr_in, sr_out)]
    assert [int(v) for v in o] == [p * M // L - W for p in range(L)]
    # the table, element by element, from the formula in float64
    for p in (0, L // 2, L - 1):
        for k in (0, W, K - 1):
            tau = (int(o[p]) + k) - p * M / L
            want = s * np.sinc(s * tau) * np.i0(12.0 * math.sqrt(1 - (tau / (W + 1)) ** 2)) / np.i0(12.0)
            assert h[p, k] == np.float32(want), (p, k)
    dev = np.abs(h.astype(np.float64).sum(1) - 1).max()
    print(f"{sr_in} -> {sr_out}: L {L} M {M} W {W} K {K}, max |sum_k h[p, k] - 1| = {dev:.2e}")
    assert dev <= 1e-5


@pytest.mark.parametrize("sr_in,sr_out", R.PAIRS, ids=R.PAIR_IDS)
def test_filter_quality(sr_in, sr_out):
    from stzs.resample import design
    ny = min(sr_in, sr_out) / 2
    pb = max(R.tone_error(design, sr_in, sr_out, f) for f in (0.0, 0.8 * ny))
    print(f"{sr_in} -> {sr_out}: passband deviation {pb:.3e}")
    assert pb <= 4 * PASSBAND_MAX
    if sr_out < sr_in:
        tones = [f * sr_out / 2 for f in (1.1, 1.2) if f * sr_out / 2 < sr_in / 2]
        assert tones or (sr_in, sr_out) == (24000, 22050)
        for f in tones:
            sb = R.tone_error(design, sr_in, sr_out, f, stop=True)
            print(f"{sr_in} -> {sr_out}: leakage at {f:.0f} Hz {sb:.3e} ({20 * math.log10(max(sb, 1e-30)):.0f} dB)")
            assert sb <= 4 * STOPBAND_MAX


def test_out_len_is_the_exact_ceiling():
    from stzs.resample import design, out_len
    for sr_in, sr_out in R.PAIRS:
        L, M = design(sr_in, sr_out)[:2]
        for n in (0, 1, M - 1, M, 10 ** 9):
            want = (n * L) // M + (1 if (n * L) % M else 0)
            assert out_len(n, L, M) == want == R.out_len_ref(n, L, M), (sr_in, sr_out, n)
    assert out_len(10 ** 9, 147, 80) == 1837500000


@pytest.mark.parametrize("sr_in,sr_out", R.PAIRS, ids=R.PAIR_IDS)
def test_span_tiles_the_output(sr_in, sr_out):
    from stzs.resample import design, out_len, span
    L, M, W, K = design(sr_in, sr_out)[:4]
    N = 1000
    for chunks in ([1] * N, [7, 300, 1, N - 308], [N]):
        assert sum(chunks) == N
        n_in = n_out = 0
        for i, c in enumerate(chunks):
            n_in += c
            final = i == len(chunks) - 1
            j0, j1 = span(n_in, final, n_out, L, M, W)
            assert j0 == n_out and j1 >= j0  # no gap, no overlap
            for j in ((j0, j1 - 1) if j1 > j0 else ()):  # every emitted output has its last tap (or the end reached)
                assert final or (j * M) // L + W < n_in
            if not final:  # ... and the first one held back does not
                assert (j1 * M) // L + W >= n_in
            n_out = j1
        assert n_out == out_len(N, L, M)


def test_keyword_defaults():
    from stzs.engine import StyleTTSZS
    from stzs.scheduler import Request
    for fn, names in ((StyleTTSZS.synth, ("ref_sr", "out_sr", "out_dtype")),
                      (StyleTTSZS.synth_stream, ("ref_sr", "out_sr", "out_dtype"))):
        sig = inspect.signature(fn).parameters
        for n in names:
            assert n in sig and sig[n].default is None, (fn.__name__, n)
    assert "sr_in" in inspect.signature(StyleTTSZS.resample).parameters
    r = Request(tokens=torch.zeros(3, dtype=torch.int64), ref_wav=torch.zeros(8), noise=torch.zeros(1, 1))
    assert r.ref_sr is None and r.out_sr is None


def test_torch_operator_is_registered_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from stzs import ops
    assert "resample" in ops.OPS and hasattr(torch.ops.stzs, "resample")
    with FakeTensorMode():
        y, n = torch.ops.stzs.resample(torch.empty(3, 24001), 24000, 48000)
        assert y.shape == (3, 48002) and y.dtype == torch.float32 and n.shape == (3,) and n.dtype == torch.int32
        y, n = torch.ops.stzs.resample(torch.empty(2, 1000), 24000, 44100, torch.empty(2, dtype=torch.int32), True)
        assert y.shape == (2, 1838) and y.dtype == torch.int16 and n.dtype == torch.int32
        y, _ = torch.ops.stzs.resample(torch.empty(1, 7), 24000, 24000, None, True)
        assert y.shape == (1, 7) and y.dtype == torch.int16
    with pytest.raises(NotImplementedError):
        torch.ops.stzs.resample(torch.zeros(1, 100), 24000, 48000)  # a CPU tensor: no fallback


def test_bad_rates_raise_before_any_launch(tiny):
    from stzs.engine import StyleTTSZS
    from stzs.resample import design, ratio, resampler
    for a, b in ((0, 24000), (24000, -1), (24000, 0), (24000.0, 48000)):  # sr <= 0 (or not an integer)
        with pytest.raises(ValueError):
            ratio(a, b)
    with pytest.raises(ValueError):
        design(24000, 24001)  # L, M > 1024
    with pytest.raises(ValueError):
        design(48000, 5000)   # L = 5, M = 48: ratio > 8
    with pytest.raises(ValueError):
        resampler("cpu", 24000, 24001)
    assert ratio(48000, 6000) == (1, 8)  # (8 itself is allowed)
    eng = object.__new__(StyleTTSZS)  # no device behind it: everything below must raise before touching one
    eng.spec, eng.device, eng.launches = tiny, torch.device("cpu"), 0
    with pytest.raises(ValueError):
        eng.resample(torch.zeros(1, 10), 24000, 0)
    with pytest.raises(ValueError):
        eng._check_out(24001, None)
    with pytest.raises(ValueError):
        eng._check_out(48000, torch.float16)
    with pytest.raises(ValueError):
        eng._ref_in(torch.zeros(1, 10), 190, None, None)  # 24000 / 190: L = 2400
    assert eng.launches == 0


def test_entry_point_rejects_before_launch():
    """stzs_resample validates before any HIP call (no GPU here): NULL arguments and pointers, a misaligned table, a
    bad output type -> STZS_EINVAL; sizes out of range -> STZS_ESHAPE"""
    import ctypes as C

    from stzs import _lib
    lb = _lib.load()
    E, S = _lib.EINVAL, _lib.ESHAPE
    assert lb.stzs_resample(None, None) == E
    a = _lib.ResampleArgs()
    assert lb.stzs_resample(C.byref(a), None) == E  # required pointers NULL
    a.x, a.h, a.o, a.y = 0x1000, 0x2000, 0x3000, 0x4000
    assert lb.stzs_resample(C.byref(a), None) == S  # sizes all 0

    def ok():
        b = _lib.ResampleArgs()
        b.x, b.h, b.o, b.y = 0x1000, 0x2000, 0x3000, 0x4000
        b.n_x = b.bsx = b.n_total = 100
        b.j0, b.j1, b.bsy, b.B, b.L, b.M, b.K, b.lens_mul, b.out_dtype = 0, 200, 200, 1, 2, 1, 69, 1, _lib.F32
        return b
    for field, val, want in (("K", 0, S), ("K", 513, S), ("L", 1025, S), ("L", 0, S), ("M", 1025, S), ("M", 17, S),
                             ("j1", -1, S), ("j0", 201, S), ("B", 0, S), ("B", 65536, S), ("bsy", 199, S),
                             ("bsx", 99, S), ("n_total", -1, S), ("h", 0x2004, E), ("x", 0x1002, E), ("y", 0x4002, E),
                             ("o", 0x3001, E), ("lens", 0x5002, E), ("out_lens", 0x5001, E), ("out_dtype", _lib.BF16, E),
                             ("h", 0, E)):
        b = ok()
        setattr(b, field, val)
        assert lb.stzs_resample(C.byref(b), None) == want, (field, val)
    b = ok()
    b.out_dtype, b.y = _lib.I16, 0x4002  # 16-bit output: 2-byte alignment is enough
    b.j1 = b.j0 = 5  # (an empty range with everything else valid would launch: not called here)
    b.j1 = 4
    assert lb.stzs_resample(C.byref(b), None) == S
