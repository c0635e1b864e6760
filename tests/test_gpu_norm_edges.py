"""stzs_row_layernorm and stzs_chan_stats (csrc/norm.hip, csrc/rowln.hpp) at the shapes where their index arithmetic
changes path, straight through the C ABI, against fp64.

row LayerNorm: four rows (waves) per block, so R = 1, 5 and 203 leave a partial last block; a lane holds the
8-channel vectors lane + 64 i, so C = 8 uses one lane, 64 eight lanes, 520 a second pass with one lane, 2048 all four
passes.  Channel statistics: 256-row chunks split over 8 row-lanes, four rows in flight per pass with a one-row
remainder loop (the seam is at r + 24 < r1), 256 channels per block in z.

Inputs with ld > C carry NaN in the padding columns; outputs are slices of sentinel-filled buffers."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from refops import same_bits, ulp_dist

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = 1e-5
DT = {"bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _padded(x, ld, dtype):
    """x [..., C] in a NaN-filled [..., ld] tensor of dtype"""
    t = torch.full(x.shape[:-1] + (ld,), NAN, dtype=dtype)
    t[..., :x.shape[-1]] = x.to(dtype)
    return t


# R, C, (in, out), act, gdiv, G, Bt, gadd: a pairwise selection -- every value of every column appears, and every pair
# of (R, C), (C, dtypes) and (dtypes, act)
LN_CASES = [
    (1, 8, "f32", "f32", 0, 1, True, True, 0.0),
    (1, 64, "bf16", "bf16", 1, 7, False, True, 1.0),
    (1, 520, "f32", "bf16", 0, 7, True, False, 1.0),
    (1, 2048, "f32", "f32", 1, 1, False, False, 1.0),
    (5, 8, "bf16", "bf16", 1, 7, True, False, 1.0),
    (5, 64, "f32", "bf16", 0, 1, True, True, 1.0),
    (5, 520, "f32", "f32", 1, 7, True, True, 0.0),
    (5, 2048, "bf16", "bf16", 0, 1, True, True, 1.0),
    (203, 8, "f32", "bf16", 1, 1, False, True, 1.0),
    (203, 64, "f32", "f32", 0, 7, True, True, 1.0),
    (203, 520, "bf16", "bf16", 0, 1, True, True, 0.0),
    (203, 2048, "f32", "bf16", 1, 7, True, True, 0.0),
    (203, 2048, "f32", "f32", 0, 7, True, False, 1.0),
    (5, 520, "f32", "bf16", 1, 1, False, True, 0.0),
    (1, 64, "f32", "f32", 1, 7, True, True, 0.0),
    (203, 8, "bf16", "bf16", 0, 7, True, True, 1.0),
]


@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: "-".join(str(int(v) if isinstance(v, (bool, float)) else v) for v in c))
def test_row_layernorm_edges(lib, case):
    """y[r] = act((x[r] - mu) rstd (gadd + G[r / gdiv]) + Bt[r / gdiv]) vs fp64 on the stored x.  fp32 out: max-rel
    < 1e-5 per row (test_row_layernorm's bound, row by row); bf16 out: within one bf16 ulp of the rounded reference.

    One ulp of the *result* cannot hold where x_hat g + Bt cancels to nothing: the fp32 evaluation error scales with
    terms = (|x| + |mu|) rstd |g| + |Bt|, not with the result.  At R 203, C 2048 (416k outputs) one element has
    |ref| = 6.1e-8 against terms of order 1; MI355X gives it 6 bf16 ulp off, and a plain fp32 evaluation on the CPU 3.
    So an element past one ulp must instead be within its own rounding plus the fp32 evaluation error,
    2^-8 |ref| + 64 * 2^-24 terms: the mean and the variance are sums of at most 32 in-lane additions and 6 butterfly
    steps, each rounding at most 2^-24 of a partial sum of magnitudes, and the element's own chain (x - mu, rstd, g,
    Bt, slope) adds fewer than 8.  For an element that is not cancelled below 2^-10 of its terms this admits no more
    than one bf16 ulp already does (2^-8 to 2^-7 of |ref|).  (measured on MI355X: fp32 out 1.99e-7 per-row max-rel; bf16 out
    at most 1 ulp but for that one element, which is 0.05 * 2^-24 of its terms from the reference)"""
    lb, L, dev = lib
    R, C, din, dout, act, gdiv, hasG, hasBt, gadd = case
    g = _gen("rowln", case)
    x = (torch.randn(R, C, generator=g) * 3 + 1).to(DT[din])
    ng = (R + gdiv - 1) // gdiv
    gs, bs = C + 8, C + 16
    G, Bt = torch.randn(ng, C, generator=g), torch.randn(ng, C, generator=g)
    ldx = ldy = C + 8
    xd = _padded(x, ldx, DT[din]).to(dev)
    Gd, Bd = _padded(G, gs, torch.float32).to(dev), _padded(Bt, bs, torch.float32).to(dev)
    yb = torch.full((R + 2, ldy), -777.0, dtype=DT[dout], device=dev)
    before = yb.clone()
    a = L.RowLNArgs()
    a.x, a.y = xd.data_ptr(), yb.data_ptr()
    a.G, a.Bt = Gd.data_ptr() if hasG else None, Bd.data_ptr() if hasBt else None
    a.ldx, a.ldy, a.gs, a.bs = ldx, ldy, gs, bs
    a.R, a.C, a.gdiv = R, C, gdiv
    a.in_dtype, a.out_dtype = (L.BF16 if d == "bf16" else L.F32 for d in (din, dout))
    a.act, a.gadd, a.eps, a.slope = (L.ACT_LEAKY if act else L.ACT_NONE), gadd, EPS, 0.2
    L.check(lb.stzs_row_layernorm(a, None), "rowln")
    torch.cuda.synchronize()
    keep = torch.ones_like(yb, dtype=torch.bool)
    keep[:R, :C] = False
    assert same_bits(yb[keep], before[keep]), "row_layernorm wrote outside y[:R, :C]"
    got = yb[:R, :C].cpu().contiguous()
    xx = x.double()
    grp = torch.arange(R) // gdiv
    mu, rs = xx.mean(1, keepdim=True), 1 / torch.sqrt(xx.var(1, unbiased=False, keepdim=True) + EPS)
    gg = gadd + (G.double()[grp] if hasG else torch.zeros(R, C, dtype=torch.float64))
    bt = Bt.double()[grp] if hasBt else torch.zeros(R, C, dtype=torch.float64)
    ref = (xx - mu) * rs * gg + bt
    terms = (xx.abs() + mu.abs()) * rs * gg.abs() + bt.abs()
    if act:
        ref = F.leaky_relu(ref, 0.2)
    assert bool(torch.isfinite(got.float()).all())
    if dout == "f32":
        e = ((got.double() - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-30)).max().item()
        print(f"rowln {case}: max per-row max-rel {e:.3e} (bound 1e-5)")
        assert e < 1e-5
    else:
        u = ulp_dist(got, ref.float().to(torch.bfloat16))
        err = (got.double() - ref).abs()
        cancelled = u > 1
        print(f"rowln {case}: max {u.max().item()} bf16 ulp from the rounded reference; {int(cancelled.sum())} cancelled "
              f"elements past one ulp, their max err / terms = "
              f"{(err / terms)[cancelled].max().item() * 2 ** 24 if cancelled.any() else 0:.2f} * 2^-24, "
              f"max |ref| / terms = {(ref.abs() / terms)[cancelled].max().item() if cancelled.any() else 0:.2e}")
        assert bool(((u <= 1) | (err <= 2.0 ** -8 * ref.abs() + 64 * 2.0 ** -24 * terms)).all())


@pytest.mark.parametrize("T", [7, 8, 9, 25, 32, 33, 255, 256, 257, 513])
@pytest.mark.parametrize("C", [8, 128, 264, 512])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_chan_stats_edges(lib, dtype, C, T):
    """mean within 1e-5 (|mean| + std) and rstd within 1e-5 relative of fp64, per channel (test_chan_stats's bounds,
    channel by channel); stzs_chan_stats_partial + stzs_chan_stats_final(256) give the bits of stzs_chan_stats.
    C = 264 leaves one 8-channel vector to the second 256-channel block; T around 8, 32 and 256 crosses the row-lane,
    four-rows-in-flight and chunk seams.  (measured on MI355X: mean 8.8e-8, rstd 8.3e-7)"""
    lb, L, dev = lib
    B, ld, stat_bs = 2, C + 8, C + 3
    x = (torch.randn(B, T, C, generator=_gen("stats", dtype, C, T)) * 2 + 0.5).to(DT[dtype])
    xd = _padded(x, ld, DT[dtype]).to(dev)
    nws = lb.stzs_chan_stats_workspace(B, T, C) // 4

    def run(split):
        ws = torch.full((nws + 16,), -777.0, device=dev)
        m = torch.full((B + 1, stat_bs), -777.0, device=dev)
        r = torch.full((B + 1, stat_bs), -777.0, device=dev)
        a = L.StatsArgs()
        a.x, a.mean, a.rstd, a.partial = xd.data_ptr(), m.data_ptr(), r.data_ptr(), ws.data_ptr()
        a.ld, a.bs, a.stat_bs = ld, T * ld, stat_bs
        a.B, a.T, a.C, a.dtype, a.eps = B, T, C, (L.BF16 if dtype == "bf16" else L.F32), EPS
        if split:
            L.check(lb.stzs_chan_stats_partial(a, None), "stats partial")
            L.check(lb.stzs_chan_stats_final(a, 256, None), "stats final")
        else:
            L.check(lb.stzs_chan_stats(a, None), "stats")
        torch.cuda.synchronize()
        for t in (m, r):
            assert bool((t[B:] == -777.0).all()) and bool((t[:, C:] == -777.0).all()), "stats wrote outside [B, C]"
        assert bool((ws[nws:] == -777.0).all()), "partials past the stated workspace size"
        return m[:B, :C].cpu().contiguous(), r[:B, :C].cpu().contiguous()

    m, r = run(False)
    m2, r2 = run(True)
    assert same_bits(m, m2) and same_bits(r, r2)
    xx = x.double()
    mr, vr = xx.mean(1), xx.var(1, unbiased=False)
    em = ((m.double() - mr).abs() / (mr.abs() + vr.sqrt())).max().item()
    rr = 1 / torch.sqrt(vr + EPS)
    er = ((r.double() - rr).abs() / rr).max().item()
    print(f"chan_stats {dtype} C{C} T{T}: mean err / (|mean| + std) {em:.3e}, rstd rel {er:.3e} (bounds 1e-5)")
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(r).all())
    assert em <= 1e-5
    assert er <= 1e-5
