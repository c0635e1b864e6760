"""The three kernels of the per-request controls, each against the launch it must agree with, bit for
bit: stzs_cfg_euler_rows against stzs_cfg_euler on every row alone with that row's scale as the scalar;
stzs_durations with `rate` against the CPU formula on the launch's own dsum (one fp32 division, rint, clamp) and
against the launch without it; stzs_row_scale against the CPU fp32 product."""
import ctypes as C

import pytest
import torch

import refops_controls as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


# ---- stzs_cfg_euler_rows -----------------------------------------------------------------------------------------

SCALES = [5.0, 1.0, 0.0]
S0, DSIG = 2.5, -1.75


@pytest.mark.parametrize("N", [8, 257])
def test_cfg_euler_rows_matches_scalar_launch_per_row(lib, N):
    lb, L, dev = lib
    B = len(SCALES)
    g = torch.Generator().manual_seed(N)
    x0 = torch.randn(B, N, generator=g)
    D = torch.randn(2 * B, N, generator=g)
    x = torch.cat([x0, x0]).to(dev)
    Dd = D.to(dev)
    sc = torch.tensor(SCALES, dtype=torch.float32, device=dev)
    L.check(lb.stzs_cfg_euler_rows(x.data_ptr(), Dd.data_ptr(), B, N, sc.data_ptr(), S0, DSIG, None), "cfg_euler_rows")
    got = x.cpu()
    assert torch.equal(got[:B], got[B:])  # both halves of the state are updated
    assert not torch.equal(got[:B], x0)
    for b, s in enumerate(SCALES):
        # the row alone on the scalar launch, as the engine makes it for that scale (sample_style: the CFG form iff the
        # scale differs from 1): B = 1, its conditional row then its unconditional row
        xs = torch.stack([x0[b], x0[b]]).to(dev)
        Ds = torch.stack([D[b], D[B + b]]).to(dev)
        L.check(lb.stzs_cfg_euler(xs.data_ptr(), Ds.data_ptr(), 1, N, int(s != 1.0), s, S0, DSIG, None), "cfg_euler")
        assert torch.equal(got[b], xs[0].cpu()), (b, s)
        assert torch.equal(got[B + b], xs[0].cpu()), (b, s)
    # the s = 1 row takes its D_c alone: the cfg = 0 launch on it
    b = SCALES.index(1.0)
    xs, Ds = x0[b:b + 1].clone().to(dev), D[b:b + 1].clone().to(dev)
    L.check(lb.stzs_cfg_euler(xs.data_ptr(), Ds.data_ptr(), 1, N, 0, 1.0, S0, DSIG, None), "cfg_euler")
    assert torch.equal(got[b], xs[0].cpu())
    # NULL scales are refused
    assert lb.stzs_cfg_euler_rows(x.data_ptr(), Dd.data_ptr(), B, N, None, S0, DSIG, None) == L.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), got)  # (and nothing was launched)


# ---- stzs_durations with rate ------------------------------------------------------------------------------------

B_D, T_D, NBINS = 4, 5, 8
RATES = [1.0, 0.5, 3.7, 16.0]  # (the kernel takes any positive rate; 16 exercises the clamp to 1)


def _logits():
    g = torch.Generator().manual_seed(11)
    return torch.randn(B_D, T_D, NBINS, generator=g) * 2


def _durations(lib, logits, rate=None, lens=None, override=None):
    lb, L, dev = lib
    lg = logits.to(dev).contiguous()
    dur = torch.full((B_D, T_D), -777, dtype=torch.int32, device=dev)
    dsum = torch.full((B_D, T_D), float("nan"), dtype=torch.float32, device=dev)
    keep = [lg, dur, dsum]
    a = L.DurArgs()
    a.logits, a.dur, a.dsum = lg.data_ptr(), dur.data_ptr(), dsum.data_ptr()
    a.ldl, a.bsl, a.B, a.T, a.nbins = NBINS, T_D * NBINS, B_D, T_D, NBINS
    for name, v, dt in (("rate", rate, torch.float32), ("lens", lens, torch.int32), ("override_dur", override, torch.int32)):
        if v is not None:
            t = torch.as_tensor(v, dtype=dt).to(dev).contiguous()
            keep.append(t)
            setattr(a, name, t.data_ptr())
    L.check(lb.stzs_durations(a, None), "durations")
    torch.cuda.synchronize()
    return dur.cpu(), dsum.cpu()


def test_durations_rate_is_the_cpu_formula_on_the_same_dsum(lib):
    logits = _logits()
    d0, s0 = _durations(lib, logits)
    d, s = _durations(lib, logits, rate=RATES)
    assert torch.equal(s, s0)  # dsum stays the raw sum
    want = RC.durations_with_rate(s, RATES)
    print("durations with rate", d.tolist())
    assert torch.equal(d, want)
    assert torch.equal(d[0], d0[0])  # rate 1
    assert bool((d[3] == 1).all()) and bool((d0[3] > 1).any())  # rate 16: clamped to 1 where the sum alone is not
    assert not torch.equal(d[1], d0[1])
    # rate = NULL is the launch as before (and a rate of 1 everywhere gives its bits)
    d1, s1 = _durations(lib, logits, rate=[1.0] * B_D)
    assert torch.equal(d1, d0) and torch.equal(s1, s0)


def test_durations_rate_with_lens_and_override(lib):
    logits = _logits()
    lens = [5, 2, 4, 1]
    d0, s0 = _durations(lib, logits, lens=lens)
    d, s = _durations(lib, logits, rate=RATES, lens=lens)
    assert torch.equal(s, s0)
    want = RC.durations_with_rate(s, RATES)
    for b, n in enumerate(lens):
        assert torch.equal(d[b, :n], want[b, :n]) and bool((d[b, n:] == 0).all()) and bool((s[b, n:] == 0).all())
    ov = torch.arange(B_D * T_D, dtype=torch.int32).reshape(B_D, T_D) % 7
    d, s = _durations(lib, logits, rate=RATES, override=ov)
    assert torch.equal(d, ov) and torch.equal(s, _durations(lib, logits)[1])  # forced durations win
    d, _ = _durations(lib, logits, rate=RATES, lens=lens, override=ov)
    for b, n in enumerate(lens):
        assert torch.equal(d[b, :n], ov[b, :n]) and bool((d[b, n:] == 0).all())


def test_durations_bad_rates_are_taken_as_one(lib):
    logits = _logits()
    d0, s0 = _durations(lib, logits)
    bad = [0.0, -2.0, float("nan"), float("inf")]
    assert RC.device_rate(bad) == [1.0] * 4
    d, s = _durations(lib, logits, rate=bad)
    assert torch.equal(d, d0) and torch.equal(s, s0)
    # a denormal rate: the quotient saturates, the integer stays one
    d, s = _durations(lib, logits, rate=[1e-45, 1.0, 1.0, 1.0])
    assert bool((d[0] > 0).all()) and torch.equal(d[1:], d0[1:]) and torch.equal(s, s0)


# ---- stzs_row_scale ----------------------------------------------------------------------------------------------

def _row_scale(lib, x, mul, B, T, ld, bs, off=0):
    lb, L, dev = lib
    a = L.RowScaleArgs()
    a.x, a.mul, a.ld, a.bs, a.B, a.T = x.data_ptr() + 4 * off, mul.data_ptr(), ld, bs, B, T
    L.check(lb.stzs_row_scale(C.byref(a), None), "row_scale")
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", ["strided", "aligned", "unaligned_base"])
def test_row_scale_is_the_fp32_product(lib, layout):
    """B 3, T 37: non-compact (ld 3, bs 120 with guard elements between and behind the rows), 16-byte aligned (ld 1,
    bs 40: nine whole groups of four and a single element per row, three guard elements), and ld 1 on a base 4 bytes
    off the alignment (the element-wide form)"""
    lb, L, dev = lib
    B, T = 3, 37
    ld, bs, off = {"strided": (3, 120, 0), "aligned": (1, 40, 0), "unaligned_base": (1, 40, 1)}[layout]
    g = torch.Generator().manual_seed(5)
    host = torch.randn(off + B * bs + 8, generator=g)
    mul_h = torch.tensor([float(RC.pitch_factor(p)) for p in (7.0, 0.0, -12.0)], dtype=torch.float32)
    x, mul = host.to(dev), mul_h.to(dev)
    assert x.data_ptr() % 16 == 0
    _row_scale(lib, x, mul, B, T, ld, bs, off)
    got = x.cpu()
    want = host.clone()
    for b in range(B):
        ix = off + b * bs + ld * torch.arange(T)
        want[ix] = host[ix] * mul_h[b]
    assert torch.equal(got, want)  # the rows are the product, every guard element is untouched
    assert not torch.equal(got, host)
    # factor 1.0 leaves the bits
    _row_scale(lib, x, torch.ones(B, device=dev), B, T, ld, bs, off)
    assert torch.equal(x.cpu(), want)
