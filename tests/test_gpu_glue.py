"""The glue kernels of csrc/prosody.hip and csrc/misc.hip, straight through the C ABI, against the fp64 /
sequential-fp32 restatements of tests/refops.py (checked on the CPU by tests/test_refops_glue.py).

Every destination is allocated wider and longer than the kernel should write and pre-filled with a sentinel; every
test asserts that the cells outside the documented output region keep their bits.  Inputs whose leading dimension
exceeds their width carry NaN in the padding (and in one row past the end), so a stray read shows in the result."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from refops import (adaln_expand_seq32, bf, dn_cond_ref, dwup_ref, f0n_ref, mean_rows_seq32, prprep_ref, same_bits,
                    ulp_diff)

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -777.0
DT = {"bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _embed3(x, rows, ld, c0=0, dtype=torch.float32):
    """x [B, T, C] inside a NaN-filled [B, rows, ld] tensor at column c0"""
    B, T, C = x.shape
    t = torch.full((B, rows, ld), NAN, dtype=dtype)
    t[:, :T, c0:c0 + C] = x.to(dtype)
    return t


def _embed2(x, ld, c0=0):
    """x [B, C] inside a NaN-filled fp32 [B, ld] at column c0"""
    t = torch.full((x.shape[0], ld), NAN)
    t[:, c0:c0 + x.shape[1]] = x
    return t


class _Dest:
    """a sentinel-filled device buffer, the mask of the cells a kernel may write, and the check of the rest"""

    def __init__(self, shape, dtype, dev):
        self.t = torch.full(shape, SENT, dtype=dtype, device=dev)
        self.before = self.t.clone()
        self.may = torch.zeros(shape, dtype=torch.bool, device=dev)

    def untouched(self):
        return same_bits(self.t[~self.may], self.before[~self.may])


def _dtid(L, name):
    return L.BF16 if name == "bf16" else L.F32


def _close_bf16(got, ref64):
    """within one bf16 ulp of the fp64 reference rounded to bf16"""
    return ulp_diff(got, ref64.float().to(torch.bfloat16))


# ---- stzs_predictor_prep -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cs", [20, 32])
@pytest.mark.parametrize("Ch", [8, 64])
@pytest.mark.parametrize("Lc,T", [(8, 3), (8, 8), (8, 37), (1, 5), (50, 1), (50, 173)])
@pytest.mark.parametrize("f32", [0, 1])
def test_predictor_prep(lib, f32, Lc, T, Ch, Cs):
    """h copy bit-exact; resampled columns, fp32: within 4 * 2^-24 * max|codes| of torch's fp32 CPU F.interpolate (the
    same source-index formula; the allowance is the contraction of l0 c0 + l1 c1 into an FMA); bf16: within one bf16
    ulp of that value rounded to bf16.  The distance to the fp64 prprep_ref is printed.
    (measured on MI355X: fp32 at most 0.37 of the bound; 2.4e-7 from fp64 in fp32, 7.8e-3 = bf16 rounding in bf16)"""
    lb, L, dev = lib
    B, c0 = 2, 3
    g = _gen("prprep", f32, Lc, T, Ch, Cs)
    dt = torch.float32 if f32 else torch.bfloat16
    codes = torch.randn(B, Lc, Cs, generator=g)
    h = torch.randn(B, T, Ch, generator=g).to(dt)
    ldc, ldh, ldy = c0 + Cs + 5, Ch + 8, (Ch + Cs + 7) // 8 * 8 + 8
    cd = _embed3(codes, Lc + 1, ldc, c0).to(dev)
    hd = _embed3(h, T + 1, ldh, 0, dt).to(dev)
    y = _Dest((B, T + 1, ldy), dt, dev)
    y.may[:, :T, :Ch + Cs] = True
    a = L.PrPrepArgs()
    a.codes, a.h, a.y = cd.data_ptr(), hd.data_ptr(), y.t.data_ptr()
    a.ldc, a.bsc, a.ldh, a.bsh, a.ldy, a.bsy = ldc, (Lc + 1) * ldc, ldh, (T + 1) * ldh, ldy, (T + 1) * ldy
    a.B, a.L, a.T, a.c0, a.Cs, a.Ch, a.yc0, a.f32 = B, Lc, T, c0, Cs, Ch, Ch, f32
    L.check(lb.stzs_predictor_prep(a, None), "prprep")
    torch.cuda.synchronize()
    assert y.untouched()
    got = y.t[:, :T, :Ch + Cs].cpu()
    assert same_bits(got[..., :Ch].contiguous(), h)
    t32 = F.interpolate(codes.transpose(1, 2), size=T, mode="linear", align_corners=False).transpose(1, 2)
    z = got[..., Ch:].contiguous()
    ref64 = prprep_ref(codes, h.float(), T, 0, Cs)[..., Ch:]
    print(f"prprep f32={f32} L{Lc} T{T}: max |y - fp64| = {(z.double() - ref64).abs().max().item():.3e}")
    if f32:
        d = (z - t32).abs().max().item()
        tol = 4 * 2.0 ** -24 * codes.abs().max().item()
        print(f"  max |y - torch fp32| = {d:.3e} (bound {tol:.3e})")
        assert d <= tol
    else:
        assert ulp_diff(z, t32.to(torch.bfloat16)) <= 1


# ---- stzs_adain_dwup -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [8, 20, 300])
@pytest.mark.parametrize("T", [1, 2, 37])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_adain_dwup(lib, dtype, T, C):
    """vs dwup_ref (fp64) on the same bf16-representable x: fp32 within 8 * 2^-24 * sum|terms| elementwise (the
    scale (1 + g) rstd, the shift beta - mu sc, x sc + sh, the slope, the tap product, the tap sum and the bias are
    at most eight roundings, each of a value bounded by the reference's sum of absolute terms); bf16 within one
    bf16 ulp of the rounded reference.  Row T of x is NaN: the odd output at m + 1 == T must not read it, and
    equals v[T - 1] w[2] + bias.  (measured on MI355X: fp32 at most 3.44 * 2^-24 sum|terms|; bf16 at most 1 ulp)"""
    lb, L, dev = lib
    B, slope = 2, 0.2
    g = _gen("dwup", dtype, T, C)
    dt = DT[dtype]
    x = bf(torch.randn(B, T, C, generator=g) * 2 + 0.5)
    mean, gamma, beta = (torch.randn(B, C, generator=g) * 0.5 for _ in range(3))
    rstd = torch.rand(B, C, generator=g) + 0.5
    w, wb = torch.randn(C, 3, generator=g), torch.randn(C, generator=g)
    ldx, ldy, stat_bs, boff = C + 8, C + 8, C + 5, C + 3
    gb_bs = boff + C + 4
    gb = torch.full((B, gb_bs), NAN)
    gb[:, :C], gb[:, boff:boff + C] = gamma, beta
    xd = _embed3(x, T + 1, ldx, 0, dt).to(dev)
    md, rd, gd = _embed2(mean, stat_bs).to(dev), _embed2(rstd, stat_bs).to(dev), gb.to(dev)
    wd, wbd = w.to(dev), wb.to(dev)
    y = _Dest((B, 2 * T + 1, ldy), dt, dev)
    y.may[:, :2 * T, :C] = True
    a = L.DwupArgs()
    a.x, a.y, a.mean, a.rstd, a.gb, a.w, a.wb = (t.data_ptr() for t in (xd, y.t, md, rd, gd, wd, wbd))
    a.ldx, a.bsx, a.ldy, a.bsy = ldx, (T + 1) * ldx, ldy, (2 * T + 1) * ldy
    a.stat_bs, a.gb_bs, a.gb_beta_off = stat_bs, gb_bs, boff
    a.B, a.T, a.C, a.dtype, a.slope = B, T, C, _dtid(L, dtype), slope
    L.check(lb.stzs_adain_dwup(a, None), "dwup")
    torch.cuda.synchronize()
    assert y.untouched()
    got = y.t[:, :2 * T, :C].cpu().contiguous()
    ref, terms = dwup_ref(x, mean, rstd, gamma, beta, w, wb, slope)
    assert bool(torch.isfinite(got.float()).all())
    # the last odd output, written out: v[T - 1] w[2] + bias
    v = F.leaky_relu((1 + gamma.double()) * (x[:, T - 1].double() - mean.double()) * rstd.double() + beta.double(), slope)
    last = v * w[:, 2].double() + wb.double()
    assert (ref[:, 2 * T - 1] - last).abs().max().item() < 1e-12
    if dtype == "f32":
        err = (got.double() - ref).abs()
        print(f"dwup f32 T{T} C{C}: max err / sum|terms| = {(err / terms).max().item() * 2 ** 24:.2f} * 2^-24 (bound 8)")
        assert bool((err <= 8 * 2.0 ** -24 * terms).all())
    else:
        u = _close_bf16(got, ref)
        print(f"dwup bf16 T{T} C{C}: {u} bf16 ulp from the rounded reference")
        assert u <= 1


# ---- stzs_f0n_down -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("T80", [2, 6, 514])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_f0n_down(lib, dtype, T80, two):
    """k3 s2 p1 conv of F0 and N with both borders (B = 3; T80 = 514 is 771 outputs: blocks and a tail) into column
    cf0 / cn0 of y0 and, when given, cf1 / cn1 of y1.  fp32 within 4 * 2^-24 * sum|terms| (three products, their
    sums and the bias); bf16 within one ulp of the rounded reference; y0 and y1 bit-identical.
    (measured on MI355X: fp32 at most 1.65 * 2^-24 sum|terms|)"""
    lb, L, dev = lib
    B, T40 = 3, T80 // 2
    g = _gen("f0n", dtype, T80, two)
    dt = DT[dtype]
    f0 = torch.randn(B, T80, generator=g) * 100 + 200
    nn = torch.randn(B, T80, generator=g)
    wf, wn = torch.randn(4, generator=g), torch.randn(4, generator=g)
    ldf = T80 + 3
    fd, nd = _embed2(f0, ldf).to(dev), _embed2(nn, ldf).to(dev)
    wfd, wnd = wf.to(dev), wn.to(dev)
    cf0, cn0, cf1, cn1, ld0, ld1 = 1, 5, 2, 0, 8, 11
    y0, y1 = _Dest((B, T40 + 1, ld0), dt, dev), _Dest((B, T40 + 1, ld1), dt, dev)
    y0.may[:, :T40, cf0] = y0.may[:, :T40, cn0] = True
    if two:
        y1.may[:, :T40, cf1] = y1.may[:, :T40, cn1] = True
    a = L.F0nArgs()
    a.f0, a.n, a.wf, a.wn, a.y0 = (t.data_ptr() for t in (fd, nd, wfd, wnd, y0.t))
    a.y1 = y1.t.data_ptr() if two else None
    a.ldf, a.ldy0, a.bsy0, a.ldy1, a.bsy1 = ldf, ld0, (T40 + 1) * ld0, ld1, (T40 + 1) * ld1
    a.B, a.T80, a.cf0, a.cn0, a.cf1, a.cn1, a.dtype = B, T80, cf0, cn0, cf1, cn1, _dtid(L, dtype)
    L.check(lb.stzs_f0n_down(a, None), "f0n")
    torch.cuda.synchronize()
    assert y0.untouched() and y1.untouched()
    for name, src, w4, c_0, c_1 in (("f0", f0, wf, cf0, cf1), ("n", nn, wn, cn0, cn1)):
        got = y0.t[:, :T40, c_0].cpu().contiguous()
        ref, terms = f0n_ref(src, w4)
        if dtype == "f32":
            err = (got.double() - ref).abs()
            print(f"f0n {name} f32 T80={T80}: max err / sum|terms| = {(err / terms).max().item() * 2 ** 24:.2f} * 2^-24")
            assert bool((err <= 4 * 2.0 ** -24 * terms).all())
        else:
            assert _close_bf16(got, ref) <= 1
        if two:
            assert same_bits(got, y1.t[:, :T40, c_1].cpu().contiguous())


# ---- stzs_dn_cond / _steps / _steps_f32 ----------------------------------------------------------------------------

DN_COND_F32_MEASURED = 7.2e-7  # largest |c - ref| / |ref| on MI355X over the cases below (7.165e-7, R 3, D 64, 3 steps)


def _dn_inputs(R, D, steps):
    g = _gen("dncond", R, D, steps)
    pool = (torch.rand(R, D, generator=g) * 2 - 1) * 10
    temb = (torch.rand(steps, D, generator=g) * 2 - 1) * 10
    # both sigmoid tails exactly at +-20, zero, and tiny arguments
    pool[0, :6] = torch.tensor([20.0, -20.0, 0.0, 1e-6, -1e-6, 19.5])
    temb[:, :6] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.5])
    return pool, temb


def _dn_run(lb, L, dev, form, pool, temb, R, D, steps):
    dt = torch.float32 if form == "steps_f32" else torch.bfloat16
    n = steps * R * D
    c = _Dest((n + 64,), dt, dev)
    c.may[:n] = True
    pd, td = pool.to(dev), temb.contiguous().to(dev)
    if form == "one":
        rc = lb.stzs_dn_cond(pd.data_ptr(), td.data_ptr(), c.t.data_ptr(), R, D, None)
    elif form == "steps":
        rc = lb.stzs_dn_cond_steps(pd.data_ptr(), td.data_ptr(), c.t.data_ptr(), R, D, steps, None)
    else:
        rc = lb.stzs_dn_cond_steps_f32(pd.data_ptr(), td.data_ptr(), c.t.data_ptr(), R, D, steps, None)
    L.check(rc, "dn_cond " + form)
    torch.cuda.synchronize()
    assert c.untouched()
    return c.t[:n].cpu().view(steps, R, D)


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("D", [64, 520])
@pytest.mark.parametrize("R", [1, 3])
def test_dn_cond(lib, R, D, steps):
    """c[s, r, j] = silu(pool[r, j] + temb[s, j]), arguments over +-20 (both sigmoid tails).  bf16 forms within one
    ulp of the rounded fp64 reference; the fp32 form within a relative 2 * DN_COND_F32_MEASURED of it (device expf
    and the division are not libm's; the measured maximum must itself stay under 1e-6: measured 7.2e-7 on MI355X).  steps = 1 of the _steps form
    has the bits of stzs_dn_cond, and step s of a multi-step launch those of a one-step launch on temb[s]."""
    lb, L, dev = lib
    pool, temb = _dn_inputs(R, D, steps)
    ref = dn_cond_ref(pool, temb)
    cb = _dn_run(lb, L, dev, "steps", pool, temb, R, D, steps)
    assert _close_bf16(cb, ref) <= 1
    cf = _dn_run(lb, L, dev, "steps_f32", pool, temb, R, D, steps)
    err = (cf.double() - ref).abs()
    rel = (err / ref.abs().clamp_min(1e-300)).max().item()
    print(f"dn_cond f32 R{R} D{D} steps{steps}: max relative error {rel:.3e}")
    assert rel <= 1e-6
    assert bool((err <= 2 * DN_COND_F32_MEASURED * ref.abs()).all())
    for s in range(steps):
        one = _dn_run(lb, L, dev, "one", pool, temb[s:s + 1], R, D, 1)
        assert same_bits(one, cb[s:s + 1].contiguous())
        assert same_bits(_dn_run(lb, L, dev, "steps", pool, temb[s:s + 1], R, D, 1), one)
        assert same_bits(_dn_run(lb, L, dev, "steps_f32", pool, temb[s:s + 1], R, D, 1), cf[s:s + 1].contiguous())


# ---- stzs_adaln_expand ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nchunk", [1, 6, 32])
@pytest.mark.parametrize("D", [64, 72])
@pytest.mark.parametrize("R", [1, 3])
def test_adaln_expand(lib, R, D, nchunk):
    """out[l, r, j] = mod[r, j] + table[l, j] (+ 1 where chunk j / D is in scale_mask), bit-exact vs the sequential
    fp32 restatement, for nlayers in {1, 3}, three masks, with and without the table"""
    lb, L, dev = lib
    g = _gen("adaln", R, D, nchunk)
    W = nchunk * D
    mod = torch.randn(R, W, generator=g)
    tab3 = torch.randn(3, W, generator=g)
    md = mod.to(dev)
    for nl in (1, 3):
        td = tab3[:nl].contiguous().to(dev)
        for mask in (0, 0b010010, 0xFFFFFFFF):
            for with_table in (False, True):
                n = nl * R * W
                out = _Dest((n + 64,), torch.float32, dev)
                out.may[:n] = True
                L.check(lb.stzs_adaln_expand(md.data_ptr(), td.data_ptr() if with_table else None, out.t.data_ptr(),
                                             R, D, nchunk, nl, mask, None), "adaln_expand")
                torch.cuda.synchronize()
                assert out.untouched()
                want = adaln_expand_seq32(mod, tab3[:nl] if with_table else None, D, nl, mask)
                assert same_bits(out.t[:n].cpu().view(nl, R, W), want), (nl, hex(mask), with_table)


# ---- stzs_state_init -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N", [(1, 1), (3, 85), (2, 128), (1, 257), (2, 650)])
@pytest.mark.parametrize("cfg", [0, 1])
def test_state_init(lib, cfg, B, N):
    """x = eps * sigma in fp32, bit-exact; with cfg the second half repeats the first, without it nothing past
    B N is written (B N in {1, 255, 256, 257, 1300})"""
    lb, L, dev = lib
    n = B * N
    eps = torch.randn(n, generator=_gen("state", cfg, B, N))
    sigma = 1.7
    x = _Dest((2 * n + 64,), torch.float32, dev)
    x.may[:2 * n if cfg else n] = True
    ed = eps.to(dev)
    L.check(lb.stzs_state_init(x.t.data_ptr(), ed.data_ptr(), B, N, cfg, sigma, None), "state_init")
    torch.cuda.synchronize()
    assert x.untouched()
    want = eps * torch.tensor(sigma, dtype=torch.float32)
    got = x.t.cpu()
    assert same_bits(got[:n].contiguous(), want)
    if cfg:
        assert same_bits(got[n:2 * n].contiguous(), want)


# ---- stzs_mean_rows ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c0", [0, 5])
@pytest.mark.parametrize("C", [13, 300])
@pytest.mark.parametrize("Lr", [1, 7, 8, 9, 50])
def test_mean_rows(lib, Lr, C, c0):
    """y[b, c] = mean_l x[b, l, c0 + c]: within one fp32 ulp of the rows added in order in fp32 and divided once
    (the add chain is exact by construction, only the division may differ), and within 1e-6 relative of the fp64 mean
    (positive data, so the mean is not a cancelled difference).  (measured on MI355X: 0 ulp; 3.5e-7 from fp64)"""
    lb, L, dev = lib
    B = 2
    x = torch.rand(B, Lr, C, generator=_gen("mean", Lr, C, c0)) * 3 + 0.5
    ldx, ldy = c0 + C + 3, C + 4
    xd = _embed3(x, Lr + 1, ldx, c0).to(dev)
    y = _Dest((B + 1, ldy), torch.float32, dev)
    y.may[:B, :C] = True
    L.check(lb.stzs_mean_rows(xd.data_ptr(), y.t.data_ptr(), B, Lr, ldx, (Lr + 1) * ldx, c0, C, ldy, None), "mean_rows")
    torch.cuda.synchronize()
    assert y.untouched()
    got = y.t[:B, :C].cpu().contiguous()
    u = ulp_diff(got, mean_rows_seq32(x))
    m64 = x.double().mean(1)
    rel = ((got.double() - m64).abs() / m64.abs()).max().item()
    print(f"mean_rows L{Lr} C{C} c0={c0}: {u} ulp from the sequential fp32 mean, {rel:.3e} relative from fp64")
    assert u <= 1
    assert rel <= 1e-6


# ---- stzs_copy2d ---------------------------------------------------------------------------------------------------

_SPECIAL = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20,   # RNE ties, just past one
            3.3895e38, -3.3895e38, 3.38e38,                                                  # just under bf16 max
            1e-40, -1e-40, 2.0 ** -133, 2.0 ** -126, 9.1835e-41,                              # denormals (fp32, bf16)
            0.0, -0.0]


@pytest.mark.parametrize("B,Rr,C", [(1, 1, 1), (2, 5, 13), (3, 7, 300)])
@pytest.mark.parametrize("dout", ["f32", "bf16"])
@pytest.mark.parametrize("din", ["f32", "bf16"])
def test_copy2d(lib, din, dout, B, Rr, C):
    """strided rows with dtype conversion, bit-exact vs torch's .to(dtype): round-to-nearest-even tie points, values
    just under the bf16 maximum, denormals and signed zeros included"""
    lb, L, dev = lib
    x = torch.randn(B, Rr, C, generator=_gen("copy", din, dout, B, Rr, C))
    sp = torch.tensor(_SPECIAL, dtype=torch.float32)
    n = x.numel()
    m = min(len(sp), n)
    x.view(-1)[:m] = sp[:m]               # (one element holds one special: test_copy2d_single_specials has the rest)
    if n >= 2 * m:
        x.view(-1)[n - m:] = sp[:m]       # and in the last block's tail
    x = x.to(DT[din])
    ldx, ldy = C + 3, C + 5
    xd = _embed3(x, Rr + 1, ldx, 0, DT[din]).to(dev)
    y = _Dest((B, Rr + 1, ldy), DT[dout], dev)
    y.may[:, :Rr, :C] = True
    a = L.CopyArgs()
    a.x, a.y, a.ldx, a.bsx, a.ldy, a.bsy = xd.data_ptr(), y.t.data_ptr(), ldx, (Rr + 1) * ldx, ldy, (Rr + 1) * ldy
    a.B, a.R, a.C, a.in_dtype, a.out_dtype = B, Rr, C, _dtid(L, din), _dtid(L, dout)
    L.check(lb.stzs_copy2d(a, None), "copy2d")
    torch.cuda.synchronize()
    assert y.untouched()
    assert same_bits(y.t[:, :Rr, :C].cpu().contiguous(), x.to(DT[dout]))


def test_copy2d_single_specials(lib):
    """the (1, 1, 1) shape once per special value (one element is all that shape holds)"""
    lb, L, dev = lib
    for din in ("f32", "bf16"):
        for dout in ("f32", "bf16"):
            for val in _SPECIAL:
                x = torch.tensor([val], dtype=torch.float32).to(DT[din])
                xd = x.to(dev)
                y = _Dest((4,), DT[dout], dev)
                y.may[:1] = True
                a = L.CopyArgs()
                a.x, a.y, a.ldx, a.bsx, a.ldy, a.bsy = xd.data_ptr(), y.t.data_ptr(), 1, 1, 1, 1
                a.B, a.R, a.C, a.in_dtype, a.out_dtype = 1, 1, 1, _dtid(L, din), _dtid(L, dout)
                L.check(lb.stzs_copy2d(a, None), "copy2d")
                torch.cuda.synchronize()
                assert y.untouched()
                assert same_bits(y.t[:1].cpu(), x.to(DT[dout])), (din, dout, val)


def test_copy2d_rejects_dtype_pair(lib):
    lb, L, dev = lib
    x = torch.zeros(8, dtype=torch.int32, device=dev)
    y = _Dest((8,), torch.float32, dev)
    for di, do in ((L.I32, L.F32), (L.F32, L.I32), (L.F8, L.BF16)):
        a = L.CopyArgs()
        a.x, a.y, a.ldx, a.bsx, a.ldy, a.bsy = x.data_ptr(), y.t.data_ptr(), 8, 8, 8, 8
        a.B, a.R, a.C, a.in_dtype, a.out_dtype = 1, 1, 8, di, do
        assert lb.stzs_copy2d(a, None) == L.EDTYPE
    torch.cuda.synchronize()
    assert y.untouched()


# ---- stzs_embed / stzs_embed_f32 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 520])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_embed(lib, dtype, D):
    """y[b, t, :] = emb[tok[b, t], :] (rounded to bf16 for stzs_embed), bit-exact; ids 0, V - 1 and repeats"""
    lb, L, dev = lib
    B, T, V = 2, 5, 11
    emb = torch.randn(V, D, generator=_gen("embed", dtype, D))
    tok = torch.tensor([[0, V - 1, 3, 3, 0], [V - 1, 5, 5, 1, 0]], dtype=torch.int32)
    ldy = D + 8
    y = _Dest((B * T + 1, ldy), DT[dtype], dev)
    y.may[:B * T, :D] = True
    td, ed = tok.to(dev), emb.to(dev)
    fn = lb.stzs_embed if dtype == "bf16" else lb.stzs_embed_f32
    L.check(fn(td.data_ptr(), ed.data_ptr(), y.t.data_ptr(), B, T, D, ldy, None), "embed")
    torch.cuda.synchronize()
    assert y.untouched()
    assert same_bits(y.t[:B * T, :D].cpu().contiguous(), emb[tok.view(-1).long()].to(DT[dtype]))
