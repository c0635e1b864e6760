"""The fp64 / sequential-fp32 restatements of tests/refops.py that the attention and glue GPU tests compare the
kernels with, each checked here against an independent torch formulation (CPU only)."""
import math

import pytest
import torch
import torch.nn.functional as F

import refops as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("Lq,Lk,heads,dh", [(1, 1, 2, 32), (17, 65, 2, 64), (50, 173, 4, 32)])
def test_attention_ref(Lq, Lk, heads, dh):
    g = _g(Lq * Lk)
    D = heads * dh
    q, k, v = (torch.randn(2, n, D, generator=g) for n in (Lq, Lk, Lk))
    o, mag = R.attention_ref(q, k, v, heads)
    sp = lambda t: t.double().view(2, -1, heads, dh).transpose(1, 2)
    want = F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(2, Lq, D)
    assert o.dtype == torch.float64 and (o - want).abs().max().item() < 1e-13
    # the magnitude bound is the same attention on |v|, dominates |o|, and equals it where v >= 0
    want_mag = F.scaled_dot_product_attention(sp(q), sp(k), sp(v).abs()).transpose(1, 2).reshape(2, Lq, D)
    assert (mag - want_mag).abs().max().item() < 1e-13
    assert bool((mag >= o.abs() - 1e-15).all())
    o2, mag2 = R.attention_ref(q, k, v.abs(), heads)
    assert torch.equal(o2, mag2)


def test_attention_ref_single_key_is_v():
    g = _g(1)
    q, k, v = torch.randn(2, 5, 64, generator=g), torch.randn(2, 1, 64, generator=g), torch.randn(2, 1, 64, generator=g)
    o, _ = R.attention_ref(q, k, v, 2)
    assert torch.equal(o, v.double().expand(2, 5, 64))


def _resample_explicit(c, T):
    """the source-index formula of upsample_linear1d(align_corners=False), written out in fp64"""
    B, L, C = c.shape
    out = torch.zeros(B, T, C, dtype=torch.float64)
    for t in range(T):
        src = max(L / T * (t + 0.5) - 0.5, 0.0)
        i0 = int(src)
        i1 = i0 + (1 if i0 < L - 1 else 0)
        l1 = src - i0
        out[:, t] = (1 - l1) * c[:, i0].double() + l1 * c[:, i1].double()
    return out


@pytest.mark.parametrize("L,T", [(8, 3), (8, 8), (8, 37), (1, 5), (50, 1), (50, 173)])
def test_prprep_ref(L, T):
    g = _g(L * 100 + T)
    codes = torch.randn(2, L, 40, generator=g)
    h = torch.randn(2, T, 8, generator=g)
    y = R.prprep_ref(codes, h, T, 3, 20)
    assert y.shape == (2, T, 28) and torch.equal(y[..., :8], h.double())
    assert (y[..., 8:] - _resample_explicit(codes[:, :, 3:23], T)).abs().max().item() < 1e-14
    if T == L:  # identity
        assert torch.equal(y[..., 8:], codes[:, :, 3:23].double())
    if L == 1:  # broadcast
        assert torch.equal(y[..., 8:], codes[:, :1, 3:23].double().expand(2, T, 20))


@pytest.mark.parametrize("T,C", [(1, 8), (2, 20), (37, 300)])
def test_dwup_ref(T, C):
    g = _g(T * C)
    x = torch.randn(2, T, C, generator=g)
    mean, gamma, beta = (torch.randn(2, C, generator=g) * 0.5 for _ in range(3))
    rstd = torch.rand(2, C, generator=g) + 0.5
    w, wb = torch.randn(C, 3, generator=g), torch.randn(C, generator=g)
    y, terms = R.dwup_ref(x, mean, rstd, gamma, beta, w, wb, 0.2)
    # explicit taps: y[2m] = v[m] w1 + b, y[2m + 1] = v[m + 1] w0 + v[m] w2 + b (v[T] = 0)
    v = F.leaky_relu((1 + gamma.double())[:, None] * (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
                     + beta.double()[:, None], 0.2)
    vn = torch.cat([v[:, 1:], torch.zeros(2, 1, C, dtype=torch.float64)], 1)
    wd, bd = w.double(), wb.double()
    want = torch.stack([v * wd[:, 1] + bd, vn * wd[:, 0] + v * wd[:, 2] + bd], 2).reshape(2, 2 * T, C)
    assert y.shape == (2, 2 * T, C) and (y - want).abs().max().item() < 1e-12
    assert bool((terms >= y.abs() - 1e-12).all())
    # T - 1's odd output has no right neighbour
    assert (y[:, 2 * T - 1] - (v[:, T - 1] * wd[:, 2] + bd)).abs().max().item() < 1e-12


@pytest.mark.parametrize("T80", [2, 6, 514])
def test_f0n_ref(T80):
    g = _g(T80)
    f = torch.randn(3, T80, generator=g)
    w4 = torch.randn(4, generator=g)
    y, terms = R.f0n_ref(f, w4)
    fp = F.pad(f.double(), (1, 1))
    wd = w4.double()
    want = fp[:, 0:T80:2] * wd[0] + fp[:, 1:T80 + 1:2] * wd[1] + fp[:, 2:T80 + 2:2] * wd[2] + wd[3]
    assert y.shape == (3, T80 // 2) and (y - want).abs().max().item() < 1e-13
    assert bool((terms >= y.abs() - 1e-13).all())


def test_dn_cond_ref():
    g = _g(7)
    pool = torch.randn(3, 64, generator=g) * 8
    temb = torch.randn(3, 64, generator=g) * 8
    c = R.dn_cond_ref(pool, temb)
    x = pool[None] + temb[:, None]           # fp32 sum
    want = F.silu(x.double())
    assert c.shape == (3, 3, 64)
    assert ((c - want).abs() / want.abs().clamp_min(1e-300)).max().item() < 1e-14
    assert abs(R.dn_cond_ref(torch.tensor([[20.0]]), torch.zeros(1, 1)).item() - 20.0 / (1 + math.exp(-20.0))) < 1e-14
    assert abs(R.dn_cond_ref(torch.tensor([[-20.0]]), torch.zeros(1, 1)).item() + 20.0 / (1 + math.exp(20.0))) < 1e-22


@pytest.mark.parametrize("L", [1, 7, 8, 9, 50])
def test_mean_rows_seq32(L):
    g = _g(L)
    x = torch.randn(2, L, 13, generator=g) * 3 + 1
    y = R.mean_rows_seq32(x)
    s = torch.zeros(2, 13)
    for l in range(L):
        s = s + x[:, l]                       # torch fp32, in order
    assert y.dtype == torch.float32 and torch.equal(y, s / L)
    assert ((y.double() - x.double().mean(1)).abs() / x.double().abs().mean(1)).max().item() < 1e-6


@pytest.mark.parametrize("mask", [0, 0b010010, 0xFFFFFFFF])
@pytest.mark.parametrize("with_table", [False, True])
def test_adaln_expand_seq32(mask, with_table):
    g = _g(mask & 0xFF)
    Rr, D, nchunk, nl = 3, 8, 6, 3
    mod = torch.randn(Rr, nchunk * D, generator=g)
    table = torch.randn(nl, nchunk * D, generator=g) if with_table else None
    out = R.adaln_expand_seq32(mod, table, D, nl, mask)
    want = mod[None].expand(nl, Rr, -1).clone()
    if with_table:
        want = want + table[:, None, :]
    for c in range(nchunk):
        if (mask >> c) & 1:
            want[:, :, c * D:(c + 1) * D] += 1.0
    assert out.dtype == torch.float32 and out.shape == (nl, Rr, nchunk * D) and torch.equal(out, want)


def test_ulp_helpers():
    a = torch.tensor([1.0, -1.0, 0.0, -0.0, 3.0e38])
    b = torch.tensor([1.0 + 2 ** -23, -1.0 - 2 ** -22, -0.0, 0.0, 3.0e38])
    assert R.ulp_diff(a, a) == 0 and R.ulp_diff(a, b) == 2
    ab, bb = torch.tensor([1.0, -2.0]).bfloat16(), torch.tensor([1.0 + 2 ** -7, -2.0]).bfloat16()
    assert R.ulp_diff(ab, bb) == 1
    assert R.same_bits(a, a.clone()) and not R.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    n = torch.tensor([float("nan")])
    assert R.same_bits(n, n.clone())
