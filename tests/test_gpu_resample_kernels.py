"""stzs_resample (csrc/resample.hip) through the C ABI, for every rate pair of
tests/refops_resample.py: against the float64 reference with the derived per-element bound; a ragged batch against
each row alone; any split of the output range and any sufficient window of the input against the whole, bit for bit;
Resampler.stream against the one-shot call; the 16-bit output against torch's rounding of the kernel's own fp32
output; the refusals.

Common setup: B = 4 rows whose conversion covers two full 1024-output tiles and a partial one, lens = [N, 1, W, N - 3],
the input inside a wider and longer buffer that holds NaN in front of the window and at and past every row's length
(a tap the kernel must not load would poison the output), the output over-allocated with a guard value."""
import ctypes as C

import numpy as np
import pytest
import torch

import refops_resample as R

pytestmark = pytest.mark.gpu

B = 4
PRE, POST = 5, 37   # NaN columns in front of / behind the window
GUARD = 777.0
N_OUT = 2 * 1024 + 300
# the pairs of the issue, and one whose table (320 phases x 69 taps, 93 KB) does not fit the LDS beside the span: the
# kernel then reads it from global memory -- the other code path, the same bits expected of it
KPAIRS = R.PAIRS + [(11025, 24000)]
KPAIR_IDS = R.PAIR_IDS + ["11025-24000"]


class Case:
    """one rate pair: tables on the host and the device, the NaN-framed input, the rows' lengths"""

    def __init__(self, dev, sr_in, sr_out):
        from stzs.resample import design, out_len
        self.dev = dev
        self.L, self.M, self.W, self.K, self.o, self.h = design(sr_in, sr_out)
        self.N = N = -(-N_OUT * self.M // self.L)
        self.n_out = out_len(N, self.L, self.M)
        assert self.n_out >= N_OUT
        self.lens = [N, 1, self.W, N - 3]
        self.out_lens = [out_len(n, self.L, self.M) for n in self.lens]
        g = torch.Generator().manual_seed(sr_in + 7 * sr_out)
        self.x = torch.randn(B, N, generator=g) * 0.3          # the rows' full signals (host, fp32)
        buf = torch.full((B, PRE + N + POST), float("nan"))
        for b, n in enumerate(self.lens):
            buf[b, PRE:PRE + n] = self.x[b, :n]
        self.buf = buf.to(dev)                                 # ragged: NaN from every row's length on
        full = torch.full((B, PRE + N + POST), float("nan"))
        full[:, PRE:PRE + N] = self.x
        self.full = full.to(dev)                               # uniform: every row N samples
        self.hd, self.od = torch.from_numpy(self.h).to(dev), torch.from_numpy(self.o).to(dev)
        self.lens_d = torch.tensor(self.lens, dtype=torch.int32, device=dev)


_CASES = {}


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


def case(dev, pair) -> Case:
    if pair not in _CASES:
        _CASES[pair] = Case(dev, *pair)
    return _CASES[pair]


def launch(lib, c, xbuf, y, *, x_off=PRE, x0=0, n_x=None, n_total=None, j0=0, j1=None, lens=None, lens_mul=1,
           out_lens=None, rows=None, y_off=0, expect=0, **over):
    """one stzs_resample call; xbuf / y are 2-D device tensors, the window starts at column x_off of xbuf"""
    lb, L, _ = lib
    a = L.ResampleArgs()
    es = xbuf.element_size()
    a.x = xbuf.data_ptr() + x_off * es
    a.h, a.o = c.hd.data_ptr(), c.od.data_ptr()
    a.y = y.data_ptr() + y_off * y.element_size()
    a.lens = None if lens is None else lens.data_ptr()
    a.out_lens = None if out_lens is None else out_lens.data_ptr()
    a.n_x = c.N if n_x is None else n_x
    a.n_total = c.N if n_total is None else n_total
    a.x0, a.bsx, a.j0, a.j1, a.bsy = x0, xbuf.stride(0), j0, c.n_out if j1 is None else j1, y.stride(0)
    a.B, a.L, a.M, a.K, a.lens_mul = xbuf.shape[0] if rows is None else rows, c.L, c.M, c.K, lens_mul
    a.out_dtype = L.I16 if y.dtype == torch.int16 else L.F32
    for k, v in over.items():
        setattr(a, k, v)
    assert 0 <= a.n_x <= xbuf.shape[1] - x_off  # (the window lies inside xbuf)
    assert a.j1 - a.j0 <= y.shape[1] - y_off or expect != 0
    rc = lb.stzs_resample(C.byref(a), None)
    assert rc == expect, (rc, expect)


def guarded(c, dtype=torch.float32, rows=B):
    return torch.full((rows, c.n_out + 64), GUARD if dtype == torch.float32 else 777, dtype=dtype, device=c.dev)


@pytest.fixture(scope="module")
def whole(lib):
    """the ragged batch's one-launch result per pair, computed once and shared: (y [B, n_out + 64], out_lens)"""
    done = {}

    def get(pair):
        if pair not in done:
            c = case(lib[2], pair)
            y = guarded(c)
            ol = torch.full((B,), -1, dtype=torch.int32, device=c.dev)
            launch(lib, c, c.buf, y, lens=c.lens_d, out_lens=ol)
            done[pair] = (y.cpu(), ol.cpu())
        return done[pair]
    return get


@pytest.mark.parametrize("pair", KPAIRS, ids=KPAIR_IDS)
def test_against_float64(lib, whole, pair):
    """every valid output within (K + 1) 2^-24 sum_k |h[p, k] x|: the first-order bound of a K-term fmaf chain with
    one rounding per term (each partial sum is at most the sum of the magnitudes), on the same fp32 table and input;
    no element left out.  Outputs past a row's end are exact zeros, the guard survives, out_lens is the formula."""
    c = case(lib[2], pair)
    y, ol = whole(pair)
    assert ol.tolist() == c.out_lens
    worst = 0.0
    for b, n in enumerate(c.lens):
        y64, sabs = R.resample_ref(c.x[b].numpy(), c.h, c.o, c.L, c.M, c.K, n=n)
        nb = c.out_lens[b]
        assert y64.shape[0] == nb
        got = y[b, :nb].numpy().astype(np.float64)
        assert np.isfinite(got).all(), "a tap outside the row was loaded (NaN)"
        bound = (c.K + 1) * 2.0 ** -24 * sabs
        err = np.abs(got - y64)
        assert (err <= bound).all(), (b, float((err - bound).max()))
        if nb:
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        tail = y[b, nb:c.n_out]
        assert not tail.any() and not torch.signbit(tail).any()  # exact +0.0 from the row's end on
        assert (y[b, c.n_out:] == GUARD).all()
    print(f"{pair}: K {c.K}, largest error / bound {worst:.3f}")


@pytest.mark.parametrize("pair", KPAIRS, ids=KPAIR_IDS)
def test_ragged_rows_equal_solo(lib, whole, pair):
    c = case(lib[2], pair)
    y, _ = whole(pair)
    for b, n in enumerate(c.lens):
        ys = guarded(c, rows=1)
        ol = torch.full((1,), -1, dtype=torch.int32, device=c.dev)
        # the row alone: a window of n samples of a signal of n samples, every output of it
        launch(lib, c, c.buf[b:b + 1], ys, n_x=n, n_total=n, j1=c.out_lens[b], out_lens=ol)
        assert ol.item() == c.out_lens[b]
        assert torch.equal(ys[0, :c.out_lens[b]].cpu(), y[b, :c.out_lens[b]]), (pair, b)
        assert (ys[0, c.out_lens[b]:] == GUARD).all()


@pytest.mark.parametrize("pair", [R.PAIRS[0], R.PAIRS[3], R.PAIRS[6]], ids=[R.PAIR_IDS[k] for k in (0, 3, 6)])
def test_null_lens_and_clamped_lens(lib, pair):
    c = case(lib[2], pair)
    ya, yb, yc, yd = (guarded(c) for _ in range(4))
    launch(lib, c, c.full, ya)                                              # NULL: N everywhere
    launch(lib, c, c.full, yb, lens=torch.full((B,), c.N, dtype=torch.int32, device=c.dev))
    assert torch.equal(ya, yb)
    # a length above n_total is its clamp, a negative one is 0 (the NaN behind the window is never read)
    hi = torch.tensor([c.N + 100, 2 ** 31 - 1, c.N, c.N + 1], dtype=torch.int32, device=c.dev)
    ol = torch.zeros(B, dtype=torch.int32, device=c.dev)
    launch(lib, c, c.full, yc, lens=hi, lens_mul=3, out_lens=ol)
    assert torch.equal(ya, yc) and ol.tolist() == [c.n_out] * B
    neg = torch.tensor([-5, c.N, -2 ** 31, 0], dtype=torch.int32, device=c.dev)
    launch(lib, c, c.full, yd, lens=neg, lens_mul=600, out_lens=ol)
    assert ol.tolist() == [0, c.n_out, 0, 0]
    assert torch.equal(yd[1], ya[1])
    for b in (0, 2, 3):
        assert not yd[b, :c.n_out].any() and (yd[b, c.n_out:] == GUARD).all()


@pytest.mark.parametrize("pair", KPAIRS, ids=KPAIR_IDS)
def test_output_splits_and_input_windows(lib, whole, pair):
    """any split of [0, n_out) and any window that holds the taps of its outputs give the bits of the whole"""
    c = case(lib[2], pair)
    y, _ = whole(pair)
    cuts = [0, 1, 1000, 1024, 1025, 1500, 2049, c.n_out]
    ys = guarded(c)
    for j0, j1 in zip(cuts[:-1], cuts[1:]):
        launch(lib, c, c.buf, ys, lens=c.lens_d, j0=j0, j1=j1, y_off=j0)
    assert torch.equal(ys.cpu(), y)
    # windows: exactly the taps of [j0, j1) (clipped to the signal), NaN around them
    yw = guarded(c)
    for j0, j1 in zip(cuts[:-1], cuts[1:]):
        lo = max(0, (j0 * c.M) // c.L - c.W)
        hi = min(c.N, ((j1 - 1) * c.M) // c.L + c.W + 1)
        win = torch.full((B, 3 + (hi - lo) + 3), float("nan"), device=c.dev)
        win[:, 3:3 + hi - lo] = c.buf[:, PRE + lo:PRE + hi]
        launch(lib, c, win, yw, x_off=3, x0=lo, n_x=hi - lo, lens=c.lens_d, j0=j0, j1=j1, y_off=j0)
    assert torch.equal(yw.cpu(), y)


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("pair", KPAIRS, ids=KPAIR_IDS)
def test_stream_equals_one_shot(lib, pair, ragged):
    from stzs.resample import resampler
    c = case(lib[2], pair)
    rs = resampler(c.dev, *pair)
    assert (rs.L, rs.M, rs.K) == (c.L, c.M, c.K)
    x = (c.buf if ragged else c.full)[:, PRE:PRE + c.N]
    lens = c.lens_d if ragged else None
    y, ol = rs(x, lens)
    assert y.shape == (B, c.n_out) and ol.tolist() == (c.out_lens if ragged else [c.n_out] * B)
    assert torch.isfinite(y).all()
    for chunks in ([1] * 20 + [c.N - 20], [7, 300, 1, c.N - 308], [300] * (c.N // 300) + [c.N % 300]):
        chunks = [n for n in chunks if n]
        assert sum(chunks) == c.N
        st = rs.stream(B, lens)
        parts, at, n0 = [], 0, 0
        for i, n in enumerate(chunks):
            j0, part = st.push(x[:, n0:n0 + n], final=i == len(chunks) - 1)
            assert j0 == at
            at += part.shape[1]
            n0 += n
            parts.append(part)
        assert at == c.n_out
        assert torch.equal(torch.cat(parts, 1), y), (pair, chunks[:4])
    # the last input chunk pushed without `final`, then the tail alone
    st = rs.stream(B, lens)
    j0, a = st.push(x[:, :c.N // 2])
    j1, b_ = st.push(x[:, c.N // 2:])
    j2, t = st.push(None, final=True)
    assert (j0, j1, j2) == (0, a.shape[1], a.shape[1] + b_.shape[1])
    assert torch.equal(torch.cat([a, b_, t], 1), y)


def test_pcm16_identity_ties_and_saturation(lib):
    """the identity table: y = x exactly, so 32768 x lands where the input puts it: on .5 ties (ties to even), on and
    beyond full scale"""
    dev = lib[2]
    c = case(dev, (24000, 24000))
    m = torch.arange(-40, 41, dtype=torch.float32)
    ties = (m + 0.5) / 32768.0
    big = torch.tensor([1.0, -1.0, 1.5, -1.5, 32767.5 / 32768, -32768.5 / 32768, 32766.5 / 32768, 0.0, -0.0])
    g = torch.Generator().manual_seed(5)
    vals = torch.cat([ties, big, torch.randn(c.N - ties.numel() - big.numel(), generator=g) * 0.5])
    x = vals[None].repeat(B, 1).contiguous().to(dev)
    yf, yi = guarded(c), guarded(c, torch.int16)
    launch(lib, c, x, yf, x_off=0)
    launch(lib, c, x, yi, x_off=0)
    assert torch.equal(yf[:, :c.N].cpu(), x.cpu())
    want = torch.clamp(torch.round(32768.0 * yf[:, :c.N]), -32768, 32767).to(torch.int16)
    assert torch.equal(yi[:, :c.N], want)
    assert (yi[:, c.N:] == 777).all()
    got = yi[0, :ties.numel()].cpu().tolist()
    assert got == [int(v) if int(v) % 2 == 0 else int(v) + 1 for v in m.tolist()]  # m + 0.5 -> the even neighbour
    assert yi[0, ties.numel():ties.numel() + 7].cpu().tolist() == [32767, -32768, 32767, -32768, 32767, -32768, 32766]


@pytest.mark.parametrize("pair", [R.PAIRS[0], R.PAIRS[1], R.PAIRS[3]], ids=[R.PAIR_IDS[k] for k in (0, 1, 3)])
def test_pcm16_equals_rounding_of_the_fp32_output(lib, pair):
    c = case(lib[2], pair)
    x = (c.full * 4.0).contiguous()  # (|y| beyond 1: saturation on a real filter)
    yf, yi = guarded(c), guarded(c, torch.int16)
    ol = torch.zeros(B, dtype=torch.int32, device=c.dev)
    launch(lib, c, x, yf, lens=c.lens_d)
    launch(lib, c, x, yi, lens=c.lens_d, out_lens=ol)
    want = torch.clamp(torch.round(32768.0 * yf[:, :c.n_out]), -32768, 32767).to(torch.int16)
    assert torch.equal(yi[:, :c.n_out], want)
    assert (want == 32767).any() and (want == -32768).any()
    assert (yi[:, c.n_out:] == 777).all() and ol.tolist() == c.out_lens
    for b in range(B):
        assert not yi[b, c.out_lens[b]:c.n_out].any()


def test_refusals_leave_the_output_alone(lib):
    _, L, dev = lib
    c = case(dev, (24000, 48000))
    y = guarded(c)
    launch(lib, c, c.full, y, expect=L.ESHAPE, K=0)
    launch(lib, c, c.full, y, expect=L.ESHAPE, L=1025)
    launch(lib, c, c.full, y, expect=L.ESHAPE, j0=10, j1=9)
    launch(lib, c, c.full, y, expect=L.ESHAPE, M=17)
    launch(lib, c, c.full, y, expect=L.EINVAL, h=c.hd.data_ptr() + 4)
    launch(lib, c, c.full, y, expect=L.EINVAL, out_dtype=L.BF16)
    torch.cuda.synchronize()
    assert (y == GUARD).all()
