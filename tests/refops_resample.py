"""float64 reference of the sample-rate conversion, numpy only: the polyphase sum on a given table,
the rate pairs every resampling test covers, and the filter-quality measurement of tests/test_resample_host.py."""
import numpy as np

# the rate pairs P: the model's 24 kHz to the consumers' rates, the references' rates to 24 kHz, the identity
PAIRS = [(24000, 48000), (24000, 16000), (24000, 8000), (24000, 44100), (24000, 22050),
         (16000, 24000), (44100, 24000), (48000, 24000), (24000, 24000)]
PAIR_IDS = [f"{a}-{b}" for a, b in PAIRS]


def out_len_ref(n, L, M):
    return -((-int(n) * int(L)) // int(M))  # ceil in exact integers


def resample_ref(x, h, o, L, M, K, n=None, j0=0, j1=None):
    """x [N] (any float type), h [L, >= K], o [L] -> (y64, sabs) over the outputs [j0, j1) (default: all out_len(n)):
    y64[j] = sum_k h[p, k] X[q M + o[p] + k] in float64 with X zero below 0 and from n on (n: the row's sample count,
    clamped into [0, N]); sabs[j] = sum_k |h[p, k] X[...]|.  Taps outside [0, n) are never read."""
    x = np.asarray(x)
    N = x.shape[-1]
    n = N if n is None else max(0, min(int(n), N))
    if j1 is None:
        j1 = out_len_ref(n, L, M)
    j = np.arange(j0, j1, dtype=np.int64)
    q, p = j // L, j % L
    idx = q[:, None] * M + np.asarray(o, np.int64)[p][:, None] + np.arange(K, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < n)
    xs = np.where(ok, x.astype(np.float64)[np.clip(idx, 0, max(N - 1, 0))], 0.0) if N else np.zeros(idx.shape)
    t = np.asarray(h)[p, :K].astype(np.float64) * xs
    return t.sum(1), np.abs(t).sum(1)


def tone_error(design, sr_in, sr_out, f_hz, n=8000, stop=False):
    """the conversion of cos(2 pi f t) of n input samples by design(sr_in, sr_out)'s fp32 table, in float64, away from
    the edges (4 K L / M + 50 outputs at each end): max |y - ideal| with ideal the cosine at the output rate, or
    (stop) max |y| -- the leakage of a tone the output rate cannot hold."""
    L, M, W, K, o, h = design(sr_in, sr_out)
    x = np.cos(2 * np.pi * f_hz * np.arange(n, dtype=np.float64) / sr_in)
    y, _ = resample_ref(x, h, o, L, M, K)
    e = int(4 * K * L / M + 50)
    assert y.shape[0] > 2 * e + 100
    j = np.arange(y.shape[0], dtype=np.float64)
    ref = 0.0 if stop else np.cos(2 * np.pi * f_hz * j / sr_out)
    return float(np.abs(y - ref)[e:-e].max())


def quality(design, sr_in, sr_out):
    """-> (passband deviation, stopband leakage or None): the larger of the errors at DC and at 0.8 x the lower
    Nyquist; for a downsampling pair the larger of the leakages at 1.1 x and 1.2 x the output Nyquist"""
    ny = min(sr_in, sr_out) / 2
    pb = max(tone_error(design, sr_in, sr_out, f) for f in (0.0, 0.8 * ny))
    sb = None
    if sr_out < sr_in:
        sb = max(tone_error(design, sr_in, sr_out, f * sr_out / 2, stop=True) for f in (1.1, 1.2))
    return pb, sb
