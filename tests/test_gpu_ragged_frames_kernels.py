"""Ragged frame batches at kernel level, straight through the C ABI: stzs_conv_args.t_lens /
t_lens_mul on the two conv forms that honour them (the generic conv_mfma path and the register-direct k3 block form at
its 64-row, 128-row and wide tiles), stzs_stats_args.lens / lens_mul on the four statistics entry points, and
stzs_dwup_args.lens.

The reference is always the SAME entry point launched on that row alone at T = T_b, compared bit for bit (torch.equal
on the stored values).  Input rows at or past a row's length are NaN (a read would poison the row: x, the residual),
operands are channel-offset in wider, longer buffers with non-compact statistics / gamma-beta strides, outputs are
over-allocated and filled with a guard value that must survive; output rows past a length are finite (convs) or exact
zeros (dwup); a length outside [1, T] behaves as its clamp; a NULL length pointer leaves the launch as it was."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 7.0
LENS = {"a": [200, 2, 64, 129], "b": [199, 65, 128, 63]}   # cross the 64-row chunk and the 64- / 128-row tile edges
T_CONV = 200
NAN = float("nan")


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _esz(t):
    return t.element_size()


_PACKED = {}


def _pack(dev, form, Ci, Co):
    """a k3 conv's random weights packed for the form (cached) -> ConvW with device tensors"""
    key = (form, Ci, Co)
    if key not in _PACKED:
        from stzs.weights import Arena, pack_conv
        g = torch.Generator().manual_seed(Ci * 1000 + Co)
        w = torch.randn(Co, Ci, 3, generator=g) / math.sqrt(3 * Ci)
        b = torch.randn(Co, generator=g) * 0.1
        A = Arena()
        cw = pack_conv(A, "t", w, b, frag32=form == "frag32")
        A.finalize(dev)
        cw.w, cw.b, cw._arena = A[cw.w], A[cw.b], A
        _PACKED[key] = cw
    return _PACKED[key]


class Ops:
    """the operands of one conv problem over B rows of T rows: x (NaN at and past each row's T_b rows), AdaIN
    statistics and gamma / beta, residuals at res_tdiv 1 and 2 (NaN past ceil(T_b / tdiv))"""

    def __init__(self, dev, B, T, Ci, Co, eff, dt, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.T, self.Ci, self.Co, self.dt, self.dev = B, T, Ci, Co, dt, dev
        self.xc0, self.ldx = 8, Ci + 16
        x = torch.full((B, T + 3, self.ldx), NAN)
        x[:, :T, 8:8 + Ci] = torch.randn(B, T, Ci, generator=g)
        self.res = {}
        for td in (1, 2):
            Tr = (T + td - 1) // td
            r = torch.full((B, Tr + 2, Co + 16), NAN)
            r[:, :Tr, 8:8 + Co] = torch.randn(B, Tr, Co, generator=g)
            for b, tb in enumerate(eff):
                r[b, (tb + td - 1) // td:] = NAN
            self.res[td] = r.to(dev, dt)
        for b, tb in enumerate(eff):
            x[b, tb:] = NAN
        self.x = x.to(dev, dt)
        self.sbs, self.gbs, self.boff = Ci + 24, 2 * Ci + 40, Ci + 16
        self.mean = torch.full((B, self.sbs), NAN)
        self.rstd = torch.full((B, self.sbs), NAN)
        self.gb = torch.full((B, self.gbs), NAN)
        self.mean[:, :Ci] = torch.randn(B, Ci, generator=g) * 0.1
        self.rstd[:, :Ci] = torch.rand(B, Ci, generator=g) + 0.5
        self.gb[:, :Ci] = torch.randn(B, Ci, generator=g) * 0.2
        self.gb[:, self.boff:self.boff + Ci] = torch.randn(B, Ci, generator=g) * 0.2
        self.mean, self.rstd, self.gb = self.mean.to(dev), self.rstd.to(dev), self.gb.to(dev)


def _conv(lb, cw, form, o, row0, nb, T, *, pro, lens=None, mul=0, stat=False, res_tdiv=0, alpha=1.0, flags=0):
    """one stzs_conv1d launch on rows [row0, row0 + nb) of the operands at width T
    -> (y [nb, T, Co], statistics slab [nb, nch, Co, 2] | None, stats_args for the finalise | None)"""
    lib_, L, dev = lb
    es = _esz(o.x)
    ldy = o.Co + 16
    y = torch.full((nb, T + 2, ldy), GUARD, dtype=o.dt, device=dev)
    a = L.ConvArgs()
    a.x = o.x.data_ptr() + (row0 * o.x.stride(0) + o.xc0) * es
    a.w, a.bias, a.y = cw.w.data_ptr(), cw.b.data_ptr(), y.data_ptr() + 8 * es
    a.ldx, a.bsx, a.ldy, a.bsy = o.ldx, o.x.stride(0), ldy, y.stride(0)
    a.B, a.T_in, a.T_out, a.Ci, a.Co, a.ks, a.dil, a.stride, a.pad = nb, T, T, o.Ci, o.Co, 3, 1, 1, 1
    a.ci_pad, a.co_pad, a.cic = cw.ci_pad, cw.co_pad, cw.cic
    a.in_dtype = a.out_dtype = L.BF16 if o.dt == torch.bfloat16 else L.F32
    a.pro_cscale, a.alpha, a.res_tdiv = 1.0, alpha, 1
    a.flags = flags | (L.CONV_W_FRAG32 if form == "frag32" else 0)
    if pro:
        a.pro_mode, a.pro_act, a.pro_slope = L.PRO_ADAIN, L.ACT_LEAKY, 0.2
        a.pro_mean = o.mean.data_ptr() + row0 * o.sbs * 4
        a.pro_rstd = o.rstd.data_ptr() + row0 * o.sbs * 4
        a.pro_gb = o.gb.data_ptr() + row0 * o.gbs * 4
        a.stat_bs, a.gb_bs, a.gb_beta_off = o.sbs, o.gbs, o.boff
    if res_tdiv:
        r = o.res[res_tdiv]
        a.res = r.data_ptr() + (row0 * r.stride(0) + 8) * es
        a.ldr, a.bsr, a.res_tdiv = r.stride(1), r.stride(0), res_tdiv
    slab = None
    nch = (T + 63) // 64
    sld = o.Co + 8
    if stat:
        slab = torch.full((nb, nch, sld, 2), GUARD, dtype=torch.float32, device=dev)
        a.stat_part, a.stat_ld = slab.data_ptr(), sld
    if lens is not None:
        a.t_lens, a.t_lens_mul = lens.data_ptr(), mul
    rc = lib_.stzs_conv1d(C.byref(a), None)
    assert rc == 0, f"stzs_conv1d returned {rc}"
    torch.cuda.synchronize()
    assert bool((y[:, T:] == GUARD).all()) and bool((y[:, :, :8] == GUARD).all()) and \
        bool((y[:, :, 8 + o.Co:] == GUARD).all()), "a y guard was overwritten"
    if stat:
        assert bool((slab[:, :, o.Co:] == GUARD).all()), "a statistics guard was overwritten"
    return y[:, :T, 8:8 + o.Co], (slab[:, :, :o.Co] if stat else None), (slab, sld, nch)


def _final(lb, slab_info, nb, T, Co, lens=None, mul=0):
    """stzs_chan_stats_final(chunk_rows 64) of a conv's slab -> (mean, rstd) [nb, Co]"""
    lib_, L, dev = lb
    slab, sld, _ = slab_info
    mean = torch.full((nb, sld), GUARD, device=dev)
    rstd = torch.full((nb, sld), GUARD, device=dev)
    s = L.StatsArgs()
    s.mean, s.rstd, s.partial = mean.data_ptr(), rstd.data_ptr(), slab.data_ptr()
    s.stat_bs, s.B, s.T, s.C, s.eps = sld, nb, T, sld, 1e-5
    if lens is not None:
        s.lens, s.lens_mul = lens.data_ptr(), mul
    rc = lib_.stzs_chan_stats_final(C.byref(s), 64, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return mean[:, :Co], rstd[:, :Co]


VARIANTS = [dict(), dict(stat=True), dict(res_tdiv=1, alpha=1 / math.sqrt(2)), dict(stat=True, res_tdiv=2, alpha=1 / math.sqrt(2))]


def _check_rows(lb, cw, form, o, lens, mul, T, pro, flags=0, rows=None, variants=VARIANTS):
    lib_, L, dev = lb
    eff = [min(max(n * max(mul, 1), 1), T) for n in lens]
    dl = _i32(lens, dev)
    for kw in variants:
        y, part, info = _conv(lb, cw, form, o, 0, o.B, T, pro=pro, lens=dl, mul=mul, flags=flags, **kw)
        assert bool(torch.isfinite(y.float()).all()), f"{kw}: a tail output is not finite"
        if part is not None:
            m, r = _final(lb, info, o.B, T, o.Co, dl, mul)
        for b in (range(o.B) if rows is None else rows):
            tb = eff[b]
            ys, ps, si = _conv(lb, cw, form, o, b, 1, tb, pro=pro, flags=flags, **kw)
            assert torch.equal(_bits(y[b, :tb]), _bits(ys[0])), f"{kw}: row {b} (T_b {tb}) differs from its solo launch"
            if part is not None:
                nb_ = (tb + 63) // 64
                assert torch.equal(part[b, :nb_], ps[0]), f"{kw}: row {b}: statistics partials differ"
                assert bool((part[b, nb_:] == 0).all()), f"{kw}: row {b}: chunks past T_b are not zero"
                ms, rs = _final(lb, si, 1, tb, o.Co)
                assert torch.equal(m[b], ms[0]) and torch.equal(r[b], rs[0]), f"{kw}: row {b}: mean / rstd differ"


FORMS = {"generic": ("generic", 64, 32, 0), "frag32": ("frag32", 128, 32, 0), "frag32_2chunk": ("frag32", 256, 32, 0),
         "frag32_t128": ("frag32", 256, 32, "T128")}


@pytest.mark.parametrize("pro", [True, False], ids=["adain_leaky", "none"])
@pytest.mark.parametrize("lens", list(LENS))
@pytest.mark.parametrize("name", list(FORMS))
def test_conv_t_lens(lib, name, lens, pro):
    """y rows < T_b, the partial chunks < ceil(T_b / 64) and the finalised mean / rstd equal the row's solo launch at
    T = T_b; later chunks are zero, tails finite, guards intact -- plain, with stat_part, with a residual at
    res_tdiv 1 and 2 and alpha = 1 / sqrt 2"""
    _, L, dev = lib
    form, Ci, Co, fl = FORMS[name]
    flags = L.CONV_MRFV_T128 if fl == "T128" else 0
    o = Ops(dev, 4, T_CONV, Ci, Co, LENS[lens], torch.bfloat16, 11)
    _check_rows(lib, _pack(dev, form, Ci, Co), form, o, LENS[lens], 0, T_CONV, pro, flags)


def test_conv_t_lens_generic_f32(lib):
    """the generic form on fp32 activations"""
    _, L, dev = lib
    o = Ops(dev, 4, T_CONV, 64, 32, LENS["a"], torch.float32, 12)
    _check_rows(lib, _pack(dev, "generic", 64, 32), "generic", o, LENS["a"], 1, T_CONV, True)


@pytest.mark.parametrize("name", ["generic", "frag32_2chunk"])
def test_conv_t_lens_mul2(lib, name):
    """t_lens_mul = 2: lengths in 40-fps frames on the 80-fps rows (T_b = 2 lens[b]), residual at res_tdiv 2"""
    _, L, dev = lib
    form, Ci, Co, _ = FORMS[name]
    lens = [100, 1, 32, 65]
    o = Ops(dev, 4, T_CONV, Ci, Co, [2 * n for n in lens], torch.bfloat16, 13)
    _check_rows(lib, _pack(dev, form, Ci, Co), form, o, lens, 2, T_CONV, True)


def test_conv_t_lens_wide(lib, gpu_device):
    """the register-direct wide form (256 output channels per workgroup: taken where the wide grid gives every CU two
    workgroups -- batch sized from the device's CU count): rows against their solo launches (64-row tiles)"""
    _, L, dev = lib
    ncu = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    Ci, Co, T = 256, 1024, 200
    B = -(-2 * ncu // (2 * (Co // 256)))  # wide_tiles = B * 2 * Co / 256 >= 2 ncu
    g = torch.Generator().manual_seed(5)
    lens = [200, 2, 64, 129, 199, 65, 128, 63] + torch.randint(1, 201, (B - 8,), generator=g).tolist()
    o = Ops(dev, B, T, Ci, Co, lens, torch.bfloat16, 14)
    _check_rows(lib, _pack(dev, "frag32", Ci, Co), "frag32", o, lens, 0, T, True, rows=range(8),
                variants=[dict(stat=True, res_tdiv=1, alpha=1 / math.sqrt(2))])


@pytest.mark.parametrize("name", ["generic", "frag32"])
def test_conv_t_lens_clamps_and_null(lib, name):
    """device lengths 0, T + 5 and -3 behave as 1, T and 1; NULL lengths give the bits of a launch with every length
    T (the launch as it was)"""
    _, L, dev = lib
    form, Ci, Co, _ = FORMS[name]
    cw = _pack(dev, form, Ci, Co)
    T = T_CONV
    raw, eff = [0, T + 5, 64, -3], [1, T, 64, 1]
    o = Ops(dev, 4, T, Ci, Co, eff, torch.bfloat16, 15)
    kw = dict(pro=True, stat=True, res_tdiv=1)
    y, p, _ = _conv(lib, cw, form, o, 0, 4, T, lens=_i32(raw, dev), **kw)
    yw, pw, _ = _conv(lib, cw, form, o, 0, 4, T, lens=_i32(eff, dev), **kw)
    assert torch.equal(_bits(y), _bits(yw)) and torch.equal(p, pw)
    full = Ops(dev, 4, T, Ci, Co, [T] * 4, torch.bfloat16, 16)
    y0, p0, _ = _conv(lib, cw, form, full, 0, 4, T, **kw)
    y1, p1, _ = _conv(lib, cw, form, full, 0, 4, T, lens=_i32([T] * 4, dev), **kw)
    assert torch.equal(_bits(y0), _bits(y1)) and torch.equal(p0, p1)


# ---- statistics ------------------------------------------------------------------------------------------------------

T_ST, LENS_ST = 600, [600, 1, 256, 257]   # the 256-row chunk edge crossed


def _stats_ops(dev, Cn, dt, eff, T):
    g = torch.Generator().manual_seed(Cn)
    x = torch.full((len(eff), T + 2, Cn + 8), NAN)
    x[:, :T, :Cn] = torch.randn(len(eff), T, Cn, generator=g) * 2 + 0.5
    for b, tb in enumerate(eff):
        x[b, tb:] = NAN
    return x.to(dev, dt)


def _stats(lb, x, row0, nb, T, Cn, *, lens=None, mul=0, mode="one"):
    """stzs_chan_stats (mode one), _partial + _final (two), _partial + _final_group (group) on rows [row0, row0 + nb)
    -> (mean, rstd [nb, Cn], partial slab [nb, nch, Cn, 2])"""
    lib_, L, dev = lb
    nch = (T + 255) // 256
    mean = torch.full((nb, Cn + 8), GUARD, device=dev)
    rstd = torch.full((nb, Cn + 8), GUARD, device=dev)
    ws = torch.full((nb, nch, Cn, 2), GUARD, device=dev)
    a = L.StatsArgs()
    a.x = x.data_ptr() + row0 * x.stride(0) * _esz(x)
    a.mean, a.rstd, a.partial = mean.data_ptr(), rstd.data_ptr(), ws.data_ptr()
    a.ld, a.bs, a.stat_bs, a.B, a.T, a.C, a.eps = x.stride(1), x.stride(0), Cn + 8, nb, T, Cn, 1e-5
    a.dtype = L.BF16 if x.dtype == torch.bfloat16 else L.F32
    if lens is not None:
        a.lens, a.lens_mul = lens.data_ptr(), mul
    if mode == "one":
        rc = lib_.stzs_chan_stats(C.byref(a), None)
    else:
        rc = lib_.stzs_chan_stats_partial(C.byref(a), None)
        assert rc == 0, rc
        if mode == "two":
            rc = lib_.stzs_chan_stats_final(C.byref(a), 256, None)
        else:
            arr = (L.StatsArgs * 2)()
            C.memmove(C.byref(arr[0]), C.byref(a), C.sizeof(a))
            C.memmove(C.byref(arr[1]), C.byref(a), C.sizeof(a))
            m2, r2 = torch.empty_like(mean), torch.empty_like(rstd)
            arr[1].mean, arr[1].rstd = m2.data_ptr(), r2.data_ptr()
            rc = lib_.stzs_chan_stats_final_group(arr, 2, 256, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((mean[:, Cn:] == GUARD).all()) and bool((rstd[:, Cn:] == GUARD).all())
    if mode == "group":
        assert torch.equal(m2[:, :Cn], mean[:, :Cn]) and torch.equal(r2[:, :Cn], rstd[:, :Cn])
    return mean[:, :Cn], rstd[:, :Cn], ws


@pytest.mark.parametrize("mode", ["one", "two", "group"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("Cn", [32, 264])
def test_stats_lens(lib, Cn, dt, mode):
    _, L, dev = lib
    x = _stats_ops(dev, Cn, dt, LENS_ST, T_ST)
    m, r, ws = _stats(lib, x, 0, 4, T_ST, Cn, lens=_i32(LENS_ST, dev), mode=mode)
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(r).all())
    for b, tb in enumerate(LENS_ST):
        ms, rs, wss = _stats(lib, x, b, 1, tb, Cn, mode=mode)
        assert torch.equal(m[b], ms[0]) and torch.equal(r[b], rs[0]), f"row {b} (T_b {tb}): mean / rstd differ"
        nb_ = (tb + 255) // 256
        assert torch.equal(ws[b, :nb_], wss[0]) and bool((ws[b, nb_:] == 0).all()), f"row {b}: partial chunks"


def test_stats_lens_mul_clamps_null(lib):
    """lens_mul = 2 doubles the count; 0 and T + 5 behave as 1 and T; NULL = every row at T"""
    _, L, dev = lib
    Cn, T = 32, 600
    x = _stats_ops(dev, Cn, torch.bfloat16, [600, 2, 256, 514], T)
    m, r, _ = _stats(lib, x, 0, 4, T, Cn, lens=_i32([300, 1, 128, 257], dev), mul=2)
    mw, rw, _ = _stats(lib, x, 0, 4, T, Cn, lens=_i32([600, 2, 256, 514], dev))
    assert torch.equal(m, mw) and torch.equal(r, rw)
    x = _stats_ops(dev, Cn, torch.bfloat16, [1, T, 64, 1], T)
    m, r, _ = _stats(lib, x, 0, 4, T, Cn, lens=_i32([0, T + 5, 64, -3], dev))
    mw, rw, _ = _stats(lib, x, 0, 4, T, Cn, lens=_i32([1, T, 64, 1], dev))
    assert torch.equal(m, mw) and torch.equal(r, rw) and bool(torch.isfinite(m).all())
    x = _stats_ops(dev, Cn, torch.bfloat16, [T] * 4, T)
    m, r, _ = _stats(lib, x, 0, 4, T, Cn)
    mw, rw, _ = _stats(lib, x, 0, 4, T, Cn, lens=_i32([T] * 4, dev))
    assert torch.equal(m, mw) and torch.equal(r, rw)


# ---- stzs_adain_dwup -------------------------------------------------------------------------------------------------

def _dwup(lb, x, st, row0, nb, T, Cn, lens=None):
    lib_, L, dev = lb
    mean, rstd, gb, w, wb = st
    y = torch.full((nb, 2 * T + 2, Cn + 8), GUARD, dtype=x.dtype, device=dev)
    a = L.DwupArgs()
    a.x, a.y = x.data_ptr() + row0 * x.stride(0) * _esz(x), y.data_ptr()
    a.mean, a.rstd, a.gb = (t.data_ptr() + row0 * t.stride(0) * 4 for t in (mean, rstd, gb))
    a.w, a.wb = w.data_ptr(), wb.data_ptr()
    a.ldx, a.bsx, a.ldy, a.bsy = x.stride(1), x.stride(0), y.stride(1), y.stride(0)
    a.stat_bs, a.gb_bs, a.gb_beta_off = mean.stride(0), gb.stride(0), Cn + 8
    a.B, a.T, a.C, a.slope = nb, T, Cn, 0.2
    a.dtype = L.BF16 if x.dtype == torch.bfloat16 else L.F32
    if lens is not None:
        a.lens = lens.data_ptr()
    rc = lib_.stzs_adain_dwup(C.byref(a), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((y[:, 2 * T:] == GUARD).all()) and bool((y[:, :, Cn:] == GUARD).all()), "a y guard was overwritten"
    return y[:, :2 * T, :Cn]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("Cn", [48, 264])
def test_dwup_lens(lib, Cn, dt):
    """rows < 2 T_b equal the solo launch (whose odd last row 2 T_b - 1 has no right neighbour), rows >= 2 T_b are
    exact zeros; lengths 0 / T + 5 clamp; NULL = every row at T"""
    _, L, dev = lib
    T, lens = 37, [37, 1, 20, 2]
    g = torch.Generator().manual_seed(Cn)
    x = torch.full((4, T + 2, Cn + 8), NAN)
    x[:, :T, :Cn] = torch.randn(4, T, Cn, generator=g)
    for b, tb in enumerate(lens):
        x[b, tb:] = NAN
    x = x.to(dev, dt)
    mean = (torch.randn(4, Cn + 8, generator=g) * 0.1).to(dev)
    rstd = (torch.rand(4, Cn + 8, generator=g) + 0.5).to(dev)
    gb = (torch.randn(4, 2 * Cn + 24, generator=g) * 0.2).to(dev)
    st = (mean, rstd, gb, torch.randn(Cn, 3, generator=g).to(dev), torch.randn(Cn, generator=g).to(dev))
    y = _dwup(lib, x, st, 0, 4, T, Cn, _i32(lens, dev))
    for b, tb in enumerate(lens):
        ys = _dwup(lib, x, st, b, 1, tb, Cn)
        assert torch.equal(_bits(y[b, :2 * tb]), _bits(ys[0])), f"row {b} (T_b {tb}) differs from its solo launch"
        assert bool((y[b, 2 * tb:] == 0).all()), f"row {b}: rows past 2 T_b are not exact zeros"
    yc = _dwup(lib, x, st, 0, 4, T, Cn, _i32([T + 5, 0, 20, 2], dev))
    assert torch.equal(_bits(yc), _bits(y))
    xf = torch.randn(4, T + 2, Cn + 8, generator=g).to(dev, dt)
    assert torch.equal(_bits(_dwup(lib, xf, st, 0, 4, T, Cn)), _bits(_dwup(lib, xf, st, 0, 4, T, Cn, _i32([T] * 4, dev))))
