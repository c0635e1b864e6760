"""The ragged decoder at kernel level, straight through the C ABI: stzs_conv_args.t_lens with
t_lens_rows = 1 on the three forms that honour it (the register-direct Snake convs -- single-chunk, multi-chunk narrow
and wide --, the polyphase ConvTranspose with a residual or the fused noise conv, the narrow conv_post form),
stzs_source_args.lens, stzs_istft_args.lens and stzs_frame_rows.

The reference is always the SAME entry point launched on that row alone at T = T_b, compared bit for bit (torch.equal
on the stored values).  Input rows at or past a row's length are NaN (x, res, acc_in, the harmonic-source rows, F0,
post): a read would poison the row.  Operands are channel-offset in wider, longer buffers, outputs are over-allocated
and filled with a guard value that must survive; output rows past a length are finite (convs) or exact zeros (har,
wav); a length outside its range behaves as its clamp."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 7.0
NAN = float("nan")
# the 64-row statistics chunk edge, the 128-row tile edge, a row shorter than the k11 d5 halo (25 rows a side)
LENS = {"a": [200, 2, 64, 129], "b": [199, 65, 128, 63]}
T_CONV = 200
KD = [(3, 1), (3, 5), (7, 3), (11, 1), (11, 5)]


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


_PACKED = {}


def _pack(dev, key, make):
    """random weights packed once per key -> ConvW with device tensors"""
    if key not in _PACKED:
        from stzs.weights import Arena
        A = Arena()
        cw = make(A, torch.Generator().manual_seed(sum(v for v in key if isinstance(v, int)) + len(key[0])))
        A.finalize(dev)
        cw.w, cw.b, cw._arena = A[cw.w], A[cw.b], A
        if getattr(cw, "nz32", None) is not None:
            cw.nz32 = A[cw.nz32]
        _PACKED[key] = cw
    return _PACKED[key]


def _snake_w(dev, Ci, Co, ks):
    from stzs.weights import pack_conv
    return _pack(dev, ("snake", Ci, Co, ks), lambda A, g: pack_conv(
        A, "t", torch.randn(Co, Ci, ks, generator=g) / math.sqrt(ks * Ci), torch.randn(Co, generator=g) * 0.1, frag32=True))


# ---- the register-direct Snake convs ---------------------------------------------------------------------------------

class SnakeOps:
    """x, residual and accumulate input of B rows of T rows, each NaN at and past its row's T_b rows; AdaIN statistics,
    gamma / beta and the Snake alpha"""

    def __init__(self, dev, B, T, Ci, Co, eff, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.T, self.Ci, self.Co, self.dev = B, T, Ci, Co, dev
        self.xc0, self.ldx = 8, Ci + 16

        def rows(Cn):
            t = torch.full((B, T + 3, Cn + 16), NAN)
            t[:, :T, 8:8 + Cn] = torch.randn(B, T, Cn, generator=g)
            for b, tb in enumerate(eff):
                t[b, tb:] = NAN
            return t.to(dev, torch.bfloat16)
        self.x, self.res, self.acc = rows(Ci), rows(Co), rows(Co)
        self.sbs, self.gbs, self.boff = Ci + 24, 2 * Ci + 40, Ci + 16
        mean, rstd, gb = (torch.full((B, n), NAN) for n in (self.sbs, self.sbs, self.gbs))
        mean[:, :Ci] = torch.randn(B, Ci, generator=g) * 0.1
        rstd[:, :Ci] = torch.rand(B, Ci, generator=g) + 0.5
        gb[:, :Ci] = torch.randn(B, Ci, generator=g) * 0.2
        gb[:, self.boff:self.boff + Ci] = torch.randn(B, Ci, generator=g) * 0.2
        self.mean, self.rstd, self.gb = mean.to(dev), rstd.to(dev), gb.to(dev)
        self.alpha = (torch.rand(Ci, generator=g) + 0.5).to(dev)


def _snake(lb, cw, o, row0, nb, T, ks, dil, *, lens=None, res=False, acc=False, stat=False, alpha=1.0):
    """one stzs_conv1d launch on rows [row0, row0 + nb) at width T -> (y [nb, T, Co], partials [nb, nch, Co, 2] | None)"""
    lib_, L, dev = lb
    ldy = o.Co + 16
    y = torch.full((nb, T + 2, ldy), GUARD, dtype=torch.bfloat16, device=dev)
    a = L.ConvArgs()
    a.x = o.x.data_ptr() + (row0 * o.x.stride(0) + o.xc0) * 2
    a.w, a.bias, a.y = cw.w.data_ptr(), cw.b.data_ptr(), y.data_ptr() + 8 * 2
    a.ldx, a.bsx, a.ldy, a.bsy = o.ldx, o.x.stride(0), ldy, y.stride(0)
    a.B, a.T_in, a.T_out, a.Ci, a.Co, a.ks, a.dil, a.stride, a.pad = nb, T, T, o.Ci, o.Co, ks, dil, 1, dil * (ks - 1) // 2
    a.ci_pad, a.co_pad, a.cic = cw.ci_pad, cw.co_pad, cw.cic
    a.in_dtype = a.out_dtype = L.BF16
    a.pro_cscale, a.alpha, a.beta, a.res_tdiv = 1.0, alpha, 1.0, 1
    a.flags = L.CONV_W_FRAG32
    a.pro_mode, a.pro_act, a.pro_alpha = L.PRO_ADAIN, L.ACT_SNAKE, o.alpha.data_ptr()
    a.pro_mean = o.mean.data_ptr() + row0 * o.sbs * 4
    a.pro_rstd = o.rstd.data_ptr() + row0 * o.sbs * 4
    a.pro_gb = o.gb.data_ptr() + row0 * o.gbs * 4
    a.stat_bs, a.gb_bs, a.gb_beta_off = o.sbs, o.gbs, o.boff
    if res:
        a.res = o.res.data_ptr() + (row0 * o.res.stride(0) + 8) * 2
        a.ldr, a.bsr = o.res.stride(1), o.res.stride(0)
    if acc:
        a.acc_in = o.acc.data_ptr() + (row0 * o.acc.stride(0) + 8) * 2
        a.lda, a.bsa = o.acc.stride(1), o.acc.stride(0)
    slab, nch, sld = None, (T + 63) // 64, o.Co + 8
    if stat:
        slab = torch.full((nb, nch, sld, 2), GUARD, dtype=torch.float32, device=dev)
        a.stat_part, a.stat_ld = slab.data_ptr(), sld
    if lens is not None:
        a.t_lens, a.t_lens_rows = lens.data_ptr(), 1
    rc = lib_.stzs_conv1d(C.byref(a), None)
    assert rc == 0, f"stzs_conv1d returned {rc}"
    torch.cuda.synchronize()
    assert bool((y[:, T:] == GUARD).all()) and bool((y[:, :, :8] == GUARD).all()) and \
        bool((y[:, :, 8 + o.Co:] == GUARD).all()), "a y guard was overwritten"
    if stat:
        assert bool((slab[:, :, o.Co:] == GUARD).all()), "a statistics guard was overwritten"
    return y[:, :T, 8:8 + o.Co], (slab[:, :, :o.Co] if stat else None)


SNAKE_VARIANTS = [dict(), dict(res=True, stat=True), dict(res=True, acc=True, alpha=1 / 3)]


def _check_snake(lb, cw, o, lens, T, ks, dil, rows=None):
    lib_, L, dev = lb
    eff = [min(max(n, 1), T) for n in lens]
    dl = _i32(lens, dev)
    for kw in SNAKE_VARIANTS:
        y, part = _snake(lb, cw, o, 0, o.B, T, ks, dil, lens=dl, **kw)
        assert bool(torch.isfinite(y.float()).all()), f"{kw}: a tail output is not finite"
        for b in (range(o.B) if rows is None else rows):
            tb = eff[b]
            ys, ps = _snake(lb, cw, o, b, 1, tb, ks, dil, **kw)
            assert torch.equal(_bits(y[b, :tb]), _bits(ys[0])), f"{kw}: row {b} (T_b {tb}) differs from its solo launch"
            if part is not None:
                nb_ = (tb + 63) // 64
                assert torch.equal(part[b, :nb_], ps[0]), f"{kw}: row {b}: statistics partials differ"
                assert bool((part[b, nb_:] == 0).all()), f"{kw}: row {b}: chunks past T_b are not zero"


@pytest.mark.parametrize("lens", list(LENS))
@pytest.mark.parametrize("kd", KD, ids=[f"k{k}d{d}" for k, d in KD])
@pytest.mark.parametrize("C_", [128, 256], ids=["single_chunk", "multi_chunk"])
def test_snake_conv_rows(lib, C_, kd, lens):
    """y rows < T_b and the statistics partials equal the row's solo launch at T = T_b; later partial chunks are zero,
    tails finite, guards intact -- plain, with residual + statistics, with residual + accumulate input + alpha 1/3"""
    _, L, dev = lib
    ks, dil = kd
    o = SnakeOps(dev, 4, T_CONV, C_, C_, LENS[lens], 21)
    _check_snake(lib, _snake_w(dev, C_, C_, ks), o, LENS[lens], T_CONV, ks, dil)


@pytest.mark.parametrize("kd", KD, ids=[f"k{k}d{d}" for k, d in KD])
def test_snake_conv_rows_wide(lib, kd):
    """256 -> 256 at B = 64, T = 1030: the wide form (256 output channels per workgroup); eight rows against their
    solo launches"""
    _, L, dev = lib
    ks, dil = kd
    B, T = 64, 1030
    g = torch.Generator().manual_seed(5)
    lens = [1030, 2, 64, 129, 1029, 65, 128, 897] + torch.randint(1, T + 1, (B - 8,), generator=g).tolist()
    o = SnakeOps(dev, B, T, 256, 256, lens, 22)
    _check_snake(lib, _snake_w(dev, 256, 256, ks), o, lens, T, ks, dil, rows=range(8))


def test_snake_conv_clamps_and_full(lib):
    """device lengths 0, T + 5 and -3 behave as 1, T and 1; every length T gives the bits of the launch without
    lengths"""
    _, L, dev = lib
    T, ks, dil = T_CONV, 7, 3
    cw = _snake_w(dev, 128, 128, ks)
    raw, eff = [0, T + 5, 64, -3], [1, T, 64, 1]
    o = SnakeOps(dev, 4, T, 128, 128, eff, 23)
    kw = dict(res=True, stat=True)
    y, p = _snake(lib, cw, o, 0, 4, T, ks, dil, lens=_i32(raw, dev), **kw)
    yw, pw = _snake(lib, cw, o, 0, 4, T, ks, dil, lens=_i32(eff, dev), **kw)
    assert torch.equal(_bits(y), _bits(yw)) and torch.equal(p, pw)
    full = SnakeOps(dev, 4, T, 128, 128, [T] * 4, 24)
    y0, p0 = _snake(lib, cw, full, 0, 4, T, ks, dil, **kw)
    y1, p1 = _snake(lib, cw, full, 0, 4, T, ks, dil, lens=_i32([T] * 4, dev), **kw)
    assert torch.equal(_bits(y0), _bits(y1)) and torch.equal(p0, p1)


# ---- the polyphase ConvTranspose -------------------------------------------------------------------------------------

def _ups_w(dev, Ci, Co, r, noise):
    from stzs.weights import pack_conv, pack_ups_noise

    def make(A, g):
        wu = torch.randn(Ci, Co, 2 * r, generator=g) / math.sqrt(2 * Ci)
        bu = torch.randn(Co, generator=g) * 0.1
        if not noise:
            return pack_conv(A, "u", wu, bu, ups=r, frag32=True)
        return pack_ups_noise(A, "u", wu, bu, torch.randn(Co, 22, 1, generator=g) * 0.2, torch.randn(Co, generator=g) * 0.1)
    return _pack(dev, ("ups", Ci, Co, r, noise), make)


class UpsOps:
    """x [B, T, Ci] (NaN at and past T_b), the residual [B, T r + refl, Co] and the harmonic-source rows [B, T r + refl,
    32] (22 channels, the rest zero), both NaN at and past the row's own T_b r + refl output rows"""

    def __init__(self, dev, B, T, Ci, Co, r, refl, eff, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.T, self.Ci, self.Co, self.r, self.refl = B, T, Ci, Co, r, refl
        x = torch.full((B, T + 3, Ci + 16), NAN)
        x[:, :T, 8:8 + Ci] = torch.randn(B, T, Ci, generator=g)
        To = T * r + refl
        res = torch.full((B, To + 2, Co + 16), NAN)
        res[:, :To, 8:8 + Co] = torch.randn(B, To, Co, generator=g)
        har = torch.full((B, To + 2, 32), NAN)
        har[:, :To, :22] = torch.randn(B, To, 22, generator=g)
        har[:, :To, 22:] = 0
        for b, tb in enumerate(eff):
            x[b, tb:] = NAN
            res[b, tb * r + refl:] = NAN
            har[b, tb * r + refl:] = NAN
        self.x, self.res, self.har = (t.to(dev, torch.bfloat16) for t in (x, res, har))


def _ups(lb, cw, o, row0, nb, T, noise, lens=None):
    lib_, L, dev = lb
    r, refl = o.r, o.refl
    To = T * r + refl
    ldy = o.Co + 16
    y = torch.full((nb, To + 2, ldy), GUARD, dtype=torch.bfloat16, device=dev)
    a = L.ConvArgs()
    a.x = o.x.data_ptr() + (row0 * o.x.stride(0) + 8) * 2
    a.w, a.bias, a.y = cw.w.data_ptr(), cw.b.data_ptr(), y.data_ptr() + 8 * 2
    a.ldx, a.bsx, a.ldy, a.bsy = o.x.stride(1), o.x.stride(0), ldy, y.stride(0)
    a.B, a.T_in, a.T_out, a.Ci, a.Co, a.ks, a.dil, a.stride, a.pad = nb, T, T + 1, o.Ci, o.Co, 2, 1, 1, 1
    a.ups, a.ups_pad, a.T_final, a.refl = r, r // 2, T * r, refl
    a.ci_pad, a.co_pad, a.cic = cw.ci_pad, cw.co_pad, cw.cic
    a.in_dtype = a.out_dtype = L.BF16
    a.pro_cscale, a.alpha, a.res_tdiv, a.pro_act, a.pro_slope = 1.0, 1.0, 1, L.ACT_LEAKY, 0.1
    a.flags = L.CONV_W_FRAG32 | (L.CONV_UPS_NOISE if noise else 0)
    if noise:
        a.res = o.har.data_ptr() + row0 * o.har.stride(0) * 2
        a.ldr, a.bsr, a.gate = o.har.stride(1), o.har.stride(0), cw.nz32.data_ptr()
    else:
        a.res = o.res.data_ptr() + (row0 * o.res.stride(0) + 8) * 2
        a.ldr, a.bsr = o.res.stride(1), o.res.stride(0)
    if lens is not None:
        a.t_lens, a.t_lens_rows = lens.data_ptr(), 1
    rc = lib_.stzs_conv1d(C.byref(a), None)
    assert rc == 0, f"stzs_conv1d returned {rc}"
    torch.cuda.synchronize()
    assert bool((y[:, To:] == GUARD).all()) and bool((y[:, :, :8] == GUARD).all()) and \
        bool((y[:, :, 8 + o.Co:] == GUARD).all()), "a y guard was overwritten"
    return y[:, :To, 8:8 + o.Co]


UPS_SHAPES = {"128to256_r10": (128, 256, 10, 0), "256to128_r6_refl": (256, 128, 6, 1), "384to128_r6_t64": (384, 128, 6, 0)}
UPS_LENS = {"T40": (40, [40, 1, 17, 33]), "T140": (140, [140, 64, 65, 129])}  # (T140: across the 64- / 128-row input tile)


@pytest.mark.parametrize("noise", [False, True], ids=["residual", "fused_noise"])
@pytest.mark.parametrize("tl", list(UPS_LENS))
@pytest.mark.parametrize("shape", list(UPS_SHAPES))
def test_conv_transpose_rows(lib, shape, tl, noise):
    """output rows < T_b r + refl equal the row's solo launch at T_in = T_b (whose rows near its end read the zero
    padding past its last input row); tails finite; lengths outside [1, T] clamp"""
    _, L, dev = lib
    Ci, Co, r, refl = UPS_SHAPES[shape]
    T, lens = UPS_LENS[tl]
    o = UpsOps(dev, 4, T, Ci, Co, r, refl, lens, 31)
    cw = _ups_w(dev, Ci, Co, r, noise)
    y = _ups(lib, cw, o, 0, 4, T, noise, _i32(lens, dev))
    assert bool(torch.isfinite(y.float()).all()), "a tail output is not finite"
    for b, tb in enumerate(lens):
        ys = _ups(lib, cw, o, b, 1, tb, noise)
        n = tb * r + refl
        assert torch.equal(_bits(y[b, :n]), _bits(ys[0])), f"row {b} (T_b {tb}) differs from its solo launch"
    raw = [lens[0] + 5, 0, lens[2], lens[3]]
    if lens[1] == 1:
        assert torch.equal(_bits(_ups(lib, cw, o, 0, 4, T, noise, _i32(raw, dev))), _bits(y))


# ---- conv_post on the narrow form ------------------------------------------------------------------------------------

def _post(lb, cw, x, row0, nb, T, lens=None):
    lib_, L, dev = lb
    y = torch.full((nb, T + 2, 32), GUARD, dtype=torch.float32, device=dev)
    a = L.ConvArgs()
    a.x = x.data_ptr() + (row0 * x.stride(0) + 8) * 2
    a.w, a.bias, a.y = cw.w.data_ptr(), cw.b.data_ptr(), y.data_ptr()
    a.ldx, a.bsx, a.ldy, a.bsy = x.stride(1), x.stride(0), 32, y.stride(0)
    a.B, a.T_in, a.T_out, a.Ci, a.Co, a.ks, a.dil, a.stride, a.pad = nb, T, T, 128, 22, 7, 1, 1, 3
    a.ci_pad, a.co_pad, a.cic = cw.ci_pad, cw.co_pad, cw.cic
    a.in_dtype, a.out_dtype = L.BF16, L.F32
    a.pro_cscale, a.alpha, a.res_tdiv, a.pro_act, a.pro_slope = 1.0, 1.0, 1, L.ACT_LEAKY, 0.01
    a.flags = L.CONV_W_NARROW32
    if lens is not None:
        a.t_lens, a.t_lens_rows = lens.data_ptr(), 1
    rc = lib_.stzs_conv1d(C.byref(a), None)
    assert rc == 0, f"stzs_conv1d returned {rc}"
    torch.cuda.synchronize()
    # (the narrow form stores whole 8-column vectors: zeros in [22, 24))
    assert bool((y[:, T:] == GUARD).all()) and bool((y[:, :, 24:] == GUARD).all()), "a y guard was overwritten"
    return y[:, :T, :22]


@pytest.mark.parametrize("lens", list(LENS))
def test_conv_post_rows(lib, lens):
    _, L, dev = lib
    from stzs.weights import pack_conv
    cw = _pack(dev, ("post",), lambda A, g: pack_conv(A, "p", torch.randn(22, 128, 7, generator=g) / 30,
                                                       torch.randn(22, generator=g) * 0.1, narrow32=True))
    T, ln = T_CONV, LENS[lens]
    g = torch.Generator().manual_seed(41)
    x = torch.full((4, T + 3, 144), NAN)
    x[:, :T, 8:136] = torch.randn(4, T, 128, generator=g)
    for b, tb in enumerate(ln):
        x[b, tb:] = NAN
    x = x.to(dev, torch.bfloat16)
    y = _post(lib, cw, x, 0, 4, T, _i32(ln, dev))
    assert bool(torch.isfinite(y).all())
    for b, tb in enumerate(ln):
        assert torch.equal(y[b, :tb], _post(lib, cw, x, b, 1, tb)[0]), f"row {b} (T_b {tb}) differs from its solo launch"
    if ln[1] == 2:
        assert torch.equal(_post(lib, cw, x, 0, 4, T, _i32([T + 9, 2, 64, 129], dev)), y)


# ---- harmonic source -------------------------------------------------------------------------------------------------

HOP, NFFT, HS, NH = 300, 20, 5, 9


def _source(lb, F0, seeds, mw, row0, nb, T80, lens=None):
    lib_, L, dev = lb
    Tf = T80 * HOP // HS + 1
    har = torch.full((nb, Tf + 2, 32), GUARD, dtype=torch.bfloat16, device=dev)
    pref = torch.zeros(nb, NH, T80, device=dev)
    a = L.SourceArgs()
    a.f0 = F0.data_ptr() + row0 * F0.stride(0) * 4
    a.seeds, a.merge_w, a.prefix, a.har = seeds.data_ptr() + row0 * 4, mw.data_ptr(), pref.data_ptr(), har.data_ptr()
    a.ldf, a.ldh, a.bsh = F0.stride(0), 32, har.stride(0)
    a.B, a.T80, a.hop, a.n_fft, a.hop_s, a.nh = nb, T80, HOP, NFFT, HS, NH
    a.sr, a.sine_amp, a.noise_std, a.voiced_thr, a.har_dtype = 24000.0, 0.1, 0.003, 10.0, L.BF16
    if lens is not None:
        a.lens = lens.data_ptr()
    rc = lib_.stzs_harmonic_source(C.byref(a), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((har[:, Tf:] == GUARD).all()), "a har guard row was overwritten"
    return har[:, :Tf]


def test_harmonic_source_rows(lib):
    """har rows < Tf_b equal the row alone at T80 = lens[b] (the reflection at its own last sample), the rows from
    there to the padded Tf are exact zeros; F0 past a row's frames is NaN and never read; lengths clamp into [1, T80]"""
    _, L, dev = lib
    T80, lens = 14, [14, 2, 6, 12]
    g = torch.Generator().manual_seed(51)
    F0 = torch.full((4, T80 + 2), NAN)
    F0[:, :T80] = torch.rand(4, T80, generator=g) * 300 + 80
    F0[:, 3] = 0.0  # (an unvoiced frame)
    for b, n in enumerate(lens):
        F0[b, n:] = NAN
    F0 = F0.to(dev)
    seeds = _i32([3, 4, 5, 6], dev)
    mw = (torch.randn(NH + 1, generator=g) * 0.3).to(dev)
    har = _source(lib, F0, seeds, mw, 0, 4, T80, _i32(lens, dev))
    for b, n in enumerate(lens):
        one = _source(lib, F0, seeds, mw, b, 1, n)
        Tfb = n * HOP // HS + 1
        assert bool(torch.isfinite(one.float()).all())
        assert torch.equal(_bits(har[b, :Tfb]), _bits(one[0])), f"row {b} ({n} frames) differs from its solo launch"
        assert bool((har[b, Tfb:] == 0).all()), f"row {b}: har rows past Tf_b are not exact zeros"
    assert torch.equal(_bits(_source(lib, F0, seeds, mw, 0, 4, T80, _i32([T80 + 3, 2, 6, 12], dev))), _bits(har))
    F1 = torch.nan_to_num(F0, nan=120.0)  # every row full: lengths T80 = the call without lengths
    assert torch.equal(_bits(_source(lib, F1, seeds, mw, 0, 4, T80)), _bits(_source(lib, F1, seeds, mw, 0, 4, T80, _i32([T80] * 4, dev))))


# ---- iSTFT -----------------------------------------------------------------------------------------------------------

def _istft(lb, post, row0, nb, Tf, lens=None):
    lib_, L, dev = lb
    N = (Tf - 1) * HS
    wav = torch.full((nb, N + 8), GUARD, device=dev)
    a = L.IstftArgs()
    a.post, a.wav = post.data_ptr() + row0 * post.stride(0) * 4, wav.data_ptr()
    a.ldp, a.bsp, a.bsw, a.B, a.Tf, a.n_fft, a.hop_s = post.stride(1), post.stride(0), wav.stride(0), nb, Tf, NFFT, HS
    if lens is not None:
        a.lens = lens.data_ptr()
    rc = lib_.stzs_istft(C.byref(a), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((wav[:, N:] == GUARD).all()), "a wav guard was overwritten"
    return wav[:, :N]


def test_istft_rows(lib):
    """Tf 841 over four 253-frame workgroups: lengths one below a workgroup, one just past it and one across three;
    samples < (Tf_b - 1) hop_s equal the row alone at Tf = Tf_b, the tail is exact zeros, post rows >= Tf_b (NaN) are
    not read; lengths clamp into [2, Tf]"""
    _, L, dev = lib
    Tf, lens = 841, [841, 121, 361, 254]
    g = torch.Generator().manual_seed(61)
    post = torch.full((4, Tf + 2, 24), NAN)
    post[:, :Tf, :22] = torch.randn(4, Tf, 22, generator=g)
    for b, n in enumerate(lens):
        post[b, n:] = NAN
    post = post.to(dev)
    wav = _istft(lib, post, 0, 4, Tf, _i32(lens, dev))
    for b, n in enumerate(lens):
        one = _istft(lib, post, b, 1, n)
        nb_ = (n - 1) * HS
        assert bool(torch.isfinite(one).all())
        assert torch.equal(wav[b, :nb_], one[0]), f"row {b} ({n} frames) differs from its solo launch"
        assert bool((wav[b, nb_:] == 0).all()), f"row {b}: samples past its own end are not exact zeros"
    assert torch.equal(_istft(lib, post, 0, 4, Tf, _i32([Tf + 7, 121, 361, 254], dev)), wav)
    p2 = post.clone()
    p2[1, 2:] = NAN
    w2 = _istft(lib, p2, 0, 4, Tf, _i32([841, 0, 361, 254], dev))  # (0 behaves as 2)
    assert torch.equal(w2[1, :HS], _istft(lib, p2, 1, 1, 2)[0]) and bool((w2[1, HS:] == 0).all())
    full = torch.randn(4, Tf, 24, generator=g).to(dev)
    assert torch.equal(_istft(lib, full, 0, 4, Tf), _istft(lib, full, 0, 4, Tf, _i32([Tf] * 4, dev)))


# ---- stzs_frame_rows -------------------------------------------------------------------------------------------------

def test_frame_rows(lib):
    lib_, L, dev = lib
    lens = [7, 1, 3, 6, 0, -5, 50, 2 ** 31 - 1]
    T, mul, add = 9, [2, 20, 120, 1, 2 ** 30], [0, 0, 1, -1, 5]
    out = torch.full((len(mul) + 1, len(lens)), -77, dtype=torch.int32, device=dev)
    a = L.FrameRowsArgs()
    a.lens, a.out, a.B, a.T, a.n = _i32(lens, dev).data_ptr(), out.data_ptr(), len(lens), T, len(mul)
    for k, (m, d) in enumerate(zip(mul, add)):
        a.mul[k], a.add[k] = m, d
    assert lib_.stzs_frame_rows(C.byref(a), None) == 0
    torch.cuda.synchronize()
    want = [[min(min(max(n, 1), T) * m + d, 2 ** 31 - 1) for n in lens] for m, d in zip(mul, add)]
    assert out[:len(mul)].tolist() == want
    assert bool((out[len(mul)] == -77).all()), "a guard row was overwritten"
    a.n = 9
    assert lib_.stzs_frame_rows(C.byref(a), None) == L.ESHAPE
