"""Per-row lengths on the precise conv forms at kernel level, straight through the C ABI, fp32 rows in
and out: stzs_conv_args.t_lens on the register-direct split-operand form (STZS_CONV_W_FRAG32X3, csrc/mrfx.hip: the Snake
convs and the narrow conv_post form with t_lens_rows = 1, the k3 block forms with t_lens_rows = 0) and on conv_x3
(STZS_CONV_W_X3, csrc/convx.hip: the polyphase ConvTranspose, a block conv without a register-direct weight copy, the
Snake convs).

The reference is always the SAME entry point launched on that row alone at T = T_b, compared bit for bit (torch.equal).
Operands as tests/test_gpu_ragged_decoder_kernels.py builds them: channel-offset views in wider, longer buffers, NaN at
and past each row's length in x, res and acc_in, over-allocated outputs filled with a guard value that must survive;
output rows past a length are finite; a length outside its range behaves as its clamp."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 7.0
NAN = float("nan")
# the case table (tools/dispatch_trace.py --ragged-precise-cases traces the same launches without a device)
from ragged_precise_cases import BLK_SHAPES, EPI, KD, LENS, T_CONV, X3_SNAKE_KD


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def max_rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


_PACKED = {}


def _pack(dev, key, **kw):
    """random weights packed once per key -> ConvW with device tensors (wx3: the conv_x3 streams, fx3: the mrfx blocks)"""
    if key not in _PACKED:
        from stzs.weights import Arena, pack_conv
        kind, Ci, Co, ks = key[:4]
        g = torch.Generator().manual_seed(Ci + 3 * Co + 7 * ks + len(kind))
        ups = kw.get("ups", 0)
        w = torch.randn(Ci, Co, ks, generator=g) / math.sqrt(2 * Ci) if ups else \
            torch.randn(Co, Ci, ks, generator=g) / math.sqrt(ks * Ci)
        if ks == 1 and not ups:
            w = w[:, :, 0]
        A = Arena()
        cw = pack_conv(A, "t", w, torch.randn(Co, generator=g) * 0.1, x3=True, **kw)
        A.finalize(dev)
        cw.b, cw.wx3, cw._arena = A[cw.b], A[cw.wx3], A
        cw.fx3 = A[cw.fx3] if cw.fx3 is not None else None
        _PACKED[key] = cw
    return _PACKED[key]


class Ops:
    """fp32 x [B, T, Ci], residual and accumulate input [B, Tr, Co] at channel offset 8 of wider, longer buffers, each
    NaN at and past its row's own count (eff: x rows, eff_r: residual / accumulate rows); AdaIN statistics, gamma / beta
    and the Snake alpha in padded buffers"""

    def __init__(self, dev, B, T, Ci, Co, eff, seed, Tr=None, eff_r=None):
        g = torch.Generator().manual_seed(seed)
        self.B, self.T, self.Ci, self.Co, self.dev = B, T, Ci, Co, dev
        Tr = T if Tr is None else Tr
        eff_r = eff if eff_r is None else eff_r

        def rows(Cn, Tn, ef):
            t = torch.full((B, Tn + 3, Cn + 16), NAN)
            t[:, :Tn, 8:8 + Cn] = torch.randn(B, Tn, Cn, generator=g)
            for b, tb in enumerate(ef):
                t[b, tb:] = NAN
            return t.to(dev)
        self.x, self.res, self.acc = rows(Ci, T, eff), rows(Co, Tr, eff_r), rows(Co, Tr, eff_r)
        self.sbs, self.gbs, self.boff = Ci + 24, 2 * Ci + 40, Ci + 16
        mean, rstd, gb = (torch.full((B, n), NAN) for n in (self.sbs, self.sbs, self.gbs))
        mean[:, :Ci] = torch.randn(B, Ci, generator=g) * 0.1
        rstd[:, :Ci] = torch.rand(B, Ci, generator=g) + 0.5
        gb[:, :Ci] = torch.randn(B, Ci, generator=g) * 0.2
        gb[:, self.boff:self.boff + Ci] = torch.randn(B, Ci, generator=g) * 0.2
        self.mean, self.rstd, self.gb = mean.to(dev), rstd.to(dev), gb.to(dev)
        self.alpha = (torch.rand(Ci, generator=g) + 0.5).to(dev)


def _conv(lb, cw, o, row0, nb, T, ks, dil, *, form, act, adain=True, slope=0.2, lens=None, mode=1, mul=0, res=False,
          tdiv=1, acc=False, stat=False, alpha=1.0, want=0, over=None):
    """one stzs_conv1d launch (form "fx3": STZS_CONV_W_FRAG32X3, "x3": STZS_CONV_W_X3) on rows [row0, row0 + nb) at width
    T -> (y [nb, T, Co], partials [nb, nch, Co, 2] | None); want: the expected return code (a refusal: guards intact)"""
    lib_, L, dev = lb
    ldy = o.Co + 16
    y = torch.full((nb, T + 2, ldy), GUARD, dtype=torch.float32, device=dev)
    a = L.ConvArgs()
    a.x = o.x.data_ptr() + (row0 * o.x.stride(0) + 8) * 4
    a.w = (cw.fx3 if form == "fx3" else cw.wx3).data_ptr()
    a.bias, a.y = cw.b.data_ptr(), y.data_ptr() + 8 * 4
    a.ldx, a.bsx, a.ldy, a.bsy = o.x.stride(1), o.x.stride(0), ldy, y.stride(0)
    a.B, a.T_in, a.T_out, a.Ci, a.Co, a.ks, a.dil, a.stride, a.pad = nb, T, T, o.Ci, o.Co, ks, dil, 1, dil * (ks - 1) // 2
    a.ci_pad, a.co_pad, a.cic = cw.ci_pad, cw.co_pad, (128 if form == "fx3" else 32)
    a.in_dtype = a.out_dtype = L.F32
    a.pro_cscale, a.alpha, a.beta, a.res_tdiv, a.pro_slope = 1.0, alpha, 1.0, tdiv, slope
    a.flags = L.CONV_W_FRAG32X3 if form == "fx3" else L.CONV_W_X3
    a.pro_act = act
    if act == L.ACT_SNAKE:
        a.pro_alpha = o.alpha.data_ptr()
    if adain:
        a.pro_mode = L.PRO_ADAIN
        a.pro_mean = o.mean.data_ptr() + row0 * o.sbs * 4
        a.pro_rstd = o.rstd.data_ptr() + row0 * o.sbs * 4
        a.pro_gb = o.gb.data_ptr() + row0 * o.gbs * 4
        a.stat_bs, a.gb_bs, a.gb_beta_off = o.sbs, o.gbs, o.boff
    if res:
        a.res = o.res.data_ptr() + (row0 * o.res.stride(0) + 8) * 4
        a.ldr, a.bsr = o.res.stride(1), o.res.stride(0)
    if acc:
        a.acc_in = o.acc.data_ptr() + (row0 * o.acc.stride(0) + 8) * 4
        a.lda, a.bsa = o.acc.stride(1), o.acc.stride(0)
    slab, nch, sld = None, (T + 63) // 64, o.Co + 8
    if stat:
        slab = torch.full((nb, nch, sld, 2), GUARD, dtype=torch.float32, device=dev)
        a.stat_part, a.stat_ld = slab.data_ptr(), sld
    if lens is not None:
        a.t_lens, a.t_lens_rows, a.t_lens_mul = lens.data_ptr(), mode, mul
    for f, v in (over or {}).items():
        setattr(a, f, v)
    rc = lib_.stzs_conv1d(C.byref(a), None)
    torch.cuda.synchronize()
    assert rc == want, f"stzs_conv1d returned {rc}, expected {want}"
    if want != 0:
        assert bool((y == GUARD).all()) and (slab is None or bool((slab == GUARD).all())), "a refused call wrote"
        return None, None
    assert bool((y[:, T:] == GUARD).all()) and bool((y[:, :, :8] == GUARD).all()) and \
        bool((y[:, :, 8 + o.Co:] == GUARD).all()), "a y guard was overwritten"
    if stat:
        assert bool((slab[:, :, o.Co:] == GUARD).all()), "a statistics guard was overwritten"
    return y[:, :T, 8:8 + o.Co], (slab[:, :, :o.Co] if stat else None)


def _check_rows(lb, cw, o, eff, dl, T, ks, dil, kw, solo_kw=None):
    """the batch launch with lengths against every row's solo launch at T = T_b: stored rows, statistics partials"""
    y, part = _conv(lb, cw, o, 0, o.B, T, ks, dil, lens=dl, **kw)
    assert bool(torch.isfinite(y).all()), f"{kw}: a tail output is not finite"
    skw = {k: v for k, v in kw.items() if k not in ("mode", "mul")}
    for b, tb in enumerate(eff):
        ys, ps = _conv(lb, cw, o, b, 1, tb, ks, dil, **skw)
        assert torch.equal(y[b, :tb], ys[0]), f"{kw}: row {b} (T_b {tb}) differs from its solo launch"
        if part is not None:
            nb_ = (tb + 63) // 64
            assert torch.equal(part[b, :nb_], ps[0]), f"{kw}: row {b}: statistics partials differ"
            assert bool((part[b, nb_:] == 0).all()), f"{kw}: row {b}: chunks past T_b are not exact zeros"
    return y


# ---- Snake convs, t_lens_rows = 1 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("lens", list(LENS))
@pytest.mark.parametrize("epi", list(EPI))
@pytest.mark.parametrize("kd", KD, ids=[f"k{k}d{d}" for k, d in KD])
@pytest.mark.parametrize("Ci", [128, 256], ids=["single_chunk", "multi_chunk"])
def test_mrfx_snake_rows(lib, Ci, kd, epi, lens):
    """mrfx Snake convs Ci -> 128: y rows < T_b and the statistics partials equal the row's solo launch at T = T_b;
    later partial chunks are zero, tails finite, guards intact -- each of the four epilogue combinations"""
    _, L, dev = lib
    ks, dil = kd
    ln = LENS[lens]
    o = Ops(dev, 4, T_CONV, Ci, 128, ln, 21)
    cw = _pack(dev, ("snake", Ci, 128, ks), frag32=True)
    _check_rows(lib, cw, o, ln, _i32(ln, dev), T_CONV, ks, dil,
                dict(form="fx3", act=L.ACT_SNAKE, stat=True, mode=1, **EPI[epi]))


@pytest.mark.parametrize("lens", list(LENS))
@pytest.mark.parametrize("kd", X3_SNAKE_KD, ids=[f"k{k}d{d}" for k, d in X3_SNAKE_KD])
def test_conv_x3_snake_rows(lib, kd, lens):
    """the same Snake problems on conv_x3 (the engine's route with the mrfx switch off), 128 -> 128"""
    _, L, dev = lib
    ks, dil = kd
    ln = LENS[lens]
    o = Ops(dev, 4, T_CONV, 128, 128, ln, 22)
    cw = _pack(dev, ("snake", 128, 128, ks), frag32=True)
    for epi in ("plain", "res_acc_alpha"):
        _check_rows(lib, cw, o, ln, _i32(ln, dev), T_CONV, ks, dil,
                    dict(form="x3", act=L.ACT_SNAKE, stat=True, mode=1, **EPI[epi]))


@pytest.mark.parametrize("form", ["fx3", "x3"])
def test_snake_clamps_and_full(lib, form):
    """device lengths 0, T + 5 and -3 behave as 1, T and 1; every length T gives the bits of the launch without lengths"""
    _, L, dev = lib
    T, ks, dil = T_CONV, 7, 3
    cw = _pack(dev, ("snake", 128, 128, ks), frag32=True)
    raw, eff = [0, T + 5, 64, -3], [1, T, 64, 1]
    o = Ops(dev, 4, T, 128, 128, eff, 23)
    kw = dict(form=form, act=L.ACT_SNAKE, res=True, stat=True)
    y, p = _conv(lib, cw, o, 0, 4, T, ks, dil, lens=_i32(raw, dev), **kw)
    yw, pw = _conv(lib, cw, o, 0, 4, T, ks, dil, lens=_i32(eff, dev), **kw)
    assert torch.equal(y, yw) and torch.equal(p, pw)
    full = Ops(dev, 4, T, 128, 128, [T] * 4, 24)
    y0, p0 = _conv(lib, cw, full, 0, 4, T, ks, dil, **kw)
    y1, p1 = _conv(lib, cw, full, 0, 4, T, ks, dil, lens=_i32([T] * 4, dev), **kw)
    assert torch.equal(y0, y1) and torch.equal(p0, p1)


# ---- conv_post on the narrow form, t_lens_rows = 1 -------------------------------------------------------------------

def _post(lb, cw, x, row0, nb, T, lens=None):
    lib_, L, dev = lb
    y = torch.full((nb, T + 2, 32), GUARD, dtype=torch.float32, device=dev)
    a = L.ConvArgs()
    a.x = x.data_ptr() + (row0 * x.stride(0) + 8) * 4
    a.w, a.bias, a.y = cw.fx3.data_ptr(), cw.b.data_ptr(), y.data_ptr()
    a.ldx, a.bsx, a.ldy, a.bsy = x.stride(1), x.stride(0), 32, y.stride(0)
    a.B, a.T_in, a.T_out, a.Ci, a.Co, a.ks, a.dil, a.stride, a.pad = nb, T, T, 128, 22, 7, 1, 1, 3
    a.ci_pad, a.co_pad, a.cic = cw.ci_pad, cw.co_pad, 128
    a.in_dtype = a.out_dtype = L.F32
    a.pro_cscale, a.alpha, a.res_tdiv, a.pro_act, a.pro_slope = 1.0, 1.0, 1, L.ACT_LEAKY, 0.01
    a.flags = L.CONV_W_FRAG32X3
    if lens is not None:
        a.t_lens, a.t_lens_rows = lens.data_ptr(), 1
    rc = lib_.stzs_conv1d(C.byref(a), None)
    assert rc == 0, f"stzs_conv1d returned {rc}"
    torch.cuda.synchronize()
    # (masked stores past Co = 22: the padding columns stay untouched)
    assert bool((y[:, T:] == GUARD).all()) and bool((y[:, :, 22:] == GUARD).all()), "a y guard was overwritten"
    return y[:, :T, :22]


@pytest.mark.parametrize("lens", list(LENS))
def test_mrfx_conv_post_rows(lib, lens):
    _, L, dev = lib
    cw = _pack(dev, ("post", 128, 22, 7), narrow32=True)
    T, ln = T_CONV, LENS[lens]
    g = torch.Generator().manual_seed(41)
    x = torch.full((4, T + 3, 144), NAN)
    x[:, :T, 8:136] = torch.randn(4, T, 128, generator=g)
    for b, tb in enumerate(ln):
        x[b, tb:] = NAN
    x = x.to(dev)
    y = _post(lib, cw, x, 0, 4, T, _i32(ln, dev))
    assert bool(torch.isfinite(y).all())
    for b, tb in enumerate(ln):
        assert torch.equal(y[b, :tb], _post(lib, cw, x, b, 1, tb)[0]), f"row {b} (T_b {tb}) differs from its solo launch"
    if ln[1] == 2:
        assert torch.equal(_post(lib, cw, x, 0, 4, T, _i32([T + 9, 2, 64, 129], dev)), y)


# ---- block convs, t_lens_rows = 0 ------------------------------------------------------------------------------------

def _blk_case(lb, cw, form, Ci, Co, T, fl, act, res, tdiv, mul, seed):
    """frames fl (x mul rows) of T (x mul) rows; the residual holds ceil(rows / tdiv) rows"""
    _, L, dev = lb
    Tx = T * mul
    eff = [n * mul for n in fl]
    o = Ops(dev, 4, Tx, Ci, Co, eff, seed, Tr=(Tx + tdiv - 1) // tdiv, eff_r=[(n + tdiv - 1) // tdiv for n in eff])
    kw = dict(form=form, act=act, adain=act == L.ACT_LEAKY, res=res, tdiv=tdiv, stat=True, alpha=1 / math.sqrt(2.0),
              mode=0, mul=mul)
    return _check_rows(lb, cw, o, eff, _i32(fl, dev), Tx, 3, 1, kw), o, eff


@pytest.mark.parametrize("mul", [1, 2])
@pytest.mark.parametrize("res", ["nores", "tdiv1", "tdiv2"])
@pytest.mark.parametrize("act", ["leaky", "none"])
@pytest.mark.parametrize("shape", list(BLK_SHAPES))
def test_mrfx_block_rows(lib, shape, act, res, mul):
    """the k3 LeakyReLU (AdaIN prologue) / identity block convs 256 -> 128, alpha 1 / sqrt 2, fused statistics, with and
    without a residual at t / res_tdiv, t_lens_mul 1 and 2"""
    _, L, dev = lib
    T, fl = BLK_SHAPES[shape]
    cw = _pack(dev, ("blk", 256, 128, 3), frag32=True)
    _blk_case(lib, cw, "fx3", 256, 128, T, fl, L.ACT_LEAKY if act == "leaky" else L.ACT_NONE, res != "nores",
              2 if res == "tdiv2" else 1, mul, 31)


@pytest.mark.parametrize("mul", [1, 2])
@pytest.mark.parametrize("shape", list(BLK_SHAPES))
def test_conv_x3_block_rows(lib, shape, mul):
    """a block conv whose weights have no register-direct copy (48 -> 40) on conv_x3: LeakyReLU, residual at t / 2"""
    _, L, dev = lib
    T, fl = BLK_SHAPES[shape]
    cw = _pack(dev, ("blk", 48, 40, 3))
    assert cw.fx3 is None
    _blk_case(lib, cw, "x3", 48, 40, T, fl, L.ACT_LEAKY, True, 2, mul, 32)
    _blk_case(lib, cw, "x3", 48, 40, T, fl, L.ACT_NONE, False, 1, mul, 33)


def test_block_clamps(lib):
    """frame counts 0, T + 5 and -3 behave as 1, T and 1 row(s): the clamp is of the ROW count into [1, T_in] (mrfx and
    conv_x3, residual at t / 2)"""
    _, L, dev = lib
    T = 37
    raw, fl = [0, T + 5, 20, -3], [1, T, 20, 1]
    for form, key, kw in (("fx3", ("blk", 256, 128, 3), dict(frag32=True)), ("x3", ("blk", 48, 40, 3), {})):
        cw = _pack(dev, key, **kw)
        o = Ops(dev, 4, T, key[1], key[2], fl, 34, Tr=(T + 1) // 2, eff_r=[(n + 1) // 2 for n in fl])
        ck = dict(form=form, act=L.ACT_LEAKY, res=True, tdiv=2, stat=True, alpha=0.5, mode=0, mul=1)
        y, p = _conv(lib, cw, o, 0, 4, T, 3, 1, lens=_i32(raw, dev), **ck)
        yw, pw = _conv(lib, cw, o, 0, 4, T, 3, 1, lens=_i32(fl, dev), **ck)
        assert torch.equal(y, yw) and torch.equal(p, pw), form
        # t_lens_mul 2: twice the frames, clamped into [1, T_in] as rows -- 0 and -3 frames are ONE row, 30 frames T rows
        y2, p2 = _conv(lib, cw, o, 0, 4, T, 3, 1, lens=_i32([0, 30, 10, -3], dev), **dict(ck, mul=2))
        assert torch.equal(y2, yw) and torch.equal(p2, pw), form


# ---- conv_x3 polyphase ConvTranspose, t_lens_rows = 1 ----------------------------------------------------------------

class UpsOps:
    """x [B, T, Ci] (NaN at and past T_b) and the residual [B, T r + refl, Co], NaN at and past the row's own
    T_b r + refl output rows"""

    def __init__(self, dev, B, T, Ci, Co, r, refl, eff, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.T, self.Ci, self.Co, self.r, self.refl = B, T, Ci, Co, r, refl
        x = torch.full((B, T + 3, Ci + 16), NAN)
        x[:, :T, 8:8 + Ci] = torch.randn(B, T, Ci, generator=g)
        To = T * r + refl
        res = torch.full((B, To + 2, Co + 16), NAN)
        res[:, :To, 8:8 + Co] = torch.randn(B, To, Co, generator=g)
        for b, tb in enumerate(eff):
            x[b, tb:] = NAN
            res[b, tb * r + refl:] = NAN
        self.x, self.res = x.to(dev), res.to(dev)


def _ups(lb, cw, o, row0, nb, T, lens=None):
    lib_, L, dev = lb
    r, refl = o.r, o.refl
    To = T * r + refl
    ldy = o.Co + 16
    y = torch.full((nb, To + 2, ldy), GUARD, dtype=torch.float32, device=dev)
    a = L.ConvArgs()
    a.x = o.x.data_ptr() + (row0 * o.x.stride(0) + 8) * 4
    a.w, a.bias, a.y = cw.wx3.data_ptr(), cw.b.data_ptr(), y.data_ptr() + 8 * 4
    a.ldx, a.bsx, a.ldy, a.bsy = o.x.stride(1), o.x.stride(0), ldy, y.stride(0)
    a.B, a.T_in, a.T_out, a.Ci, a.Co, a.ks, a.dil, a.stride, a.pad = nb, T, T + 1, o.Ci, o.Co, 2, 1, 1, 1
    a.ups, a.ups_pad, a.T_final, a.refl = r, r // 2, T * r, refl
    a.ci_pad, a.co_pad, a.cic = cw.ci_pad, cw.co_pad, 32
    a.in_dtype = a.out_dtype = L.F32
    a.pro_cscale, a.alpha, a.res_tdiv, a.pro_act, a.pro_slope = 1.0, 1.0, 1, L.ACT_LEAKY, 0.1
    a.flags = L.CONV_W_X3
    a.res = o.res.data_ptr() + (row0 * o.res.stride(0) + 8) * 4
    a.ldr, a.bsr = o.res.stride(1), o.res.stride(0)
    if lens is not None:
        a.t_lens, a.t_lens_rows = lens.data_ptr(), 1
    rc = lib_.stzs_conv1d(C.byref(a), None)
    assert rc == 0, f"stzs_conv1d returned {rc}"
    torch.cuda.synchronize()
    assert bool((y[:, To:] == GUARD).all()) and bool((y[:, :, :8] == GUARD).all()) and \
        bool((y[:, :, 8 + o.Co:] == GUARD).all()), "a y guard was overwritten"
    return y[:, :To, 8:8 + o.Co]


@pytest.mark.parametrize("lens", list(LENS))
@pytest.mark.parametrize("refl", [0, 1])
def test_conv_x3_transpose_rows(lib, refl, lens):
    """r = 5 (k = 10), 256 -> 128, LeakyReLU(0.1), residual: output rows < T_b r + refl equal the row's solo launch at
    T_in = T_b (whose last rows read the zero padding past its last input row); tails finite; lengths clamp"""
    _, L, dev = lib
    T, ln = T_CONV, LENS[lens]
    o = UpsOps(dev, 4, T, 256, 128, 5, refl, ln, 51)
    cw = _pack(dev, ("ups", 256, 128, 10), ups=5)
    y = _ups(lib, cw, o, 0, 4, T, _i32(ln, dev))
    assert bool(torch.isfinite(y).all()), "a tail output is not finite"
    for b, tb in enumerate(ln):
        ys = _ups(lib, cw, o, b, 1, tb)
        n = tb * 5 + refl
        assert torch.equal(y[b, :n], ys[0]), f"row {b} (T_b {tb}) differs from its solo launch"
    if ln[0] == T:
        assert torch.equal(_ups(lib, cw, o, 0, 4, T, _i32([T + 5] + ln[1:], dev)), y)


# ---- the two forms against each other --------------------------------------------------------------------------------

def test_cross_form(lib):
    """the ragged mrfx and the ragged conv_x3 outputs of one Snake problem and of one block problem agree on every valid
    row within 4e-5 of max|ref| -- the bound tests/test_gpu_precise.py holds mrfx to against conv_x3 (same arithmetic,
    another K order)"""
    _, L, dev = lib
    ln = LENS["b"]
    o = Ops(dev, 4, T_CONV, 256, 128, ln, 61)
    cw = _pack(dev, ("snake", 256, 128, 7), frag32=True)
    kw = dict(act=L.ACT_SNAKE, res=True, acc=True, alpha=1 / 3, lens=_i32(ln, dev), mode=1)
    ya, _ = _conv(lib, cw, o, 0, 4, T_CONV, 7, 3, form="fx3", **kw)
    yb, _ = _conv(lib, cw, o, 0, 4, T_CONV, 7, 3, form="x3", **kw)
    T, fl = BLK_SHAPES["T130"]
    ob = Ops(dev, 4, T, 256, 128, fl, 62)
    cb = _pack(dev, ("blk", 256, 128, 3), frag32=True)
    kb = dict(act=L.ACT_LEAKY, res=True, alpha=1 / math.sqrt(2.0), lens=_i32(fl, dev), mode=0, mul=1)
    za, _ = _conv(lib, cb, ob, 0, 4, T, 3, 1, form="fx3", **kb)
    zb, _ = _conv(lib, cb, ob, 0, 4, T, 3, 1, form="x3", **kb)
    for name, p, q, lens_ in (("snake", ya, yb, ln), ("block", za, zb, fl)):
        for b, tb in enumerate(lens_):
            e = max_rel(p[b, :tb], q[b, :tb])
            print(f"cross-form {name} row {b} (T_b {tb}): max-rel {e:.2e}")
            assert e < 4e-5, (name, b, e)


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_refusals(lib):
    """STZS_EINVAL before any launch, the output guard intact"""
    lib_, L, dev = lib
    T = 40
    ln = _i32([40, 3, 20, 9], dev)
    o = Ops(dev, 4, T, 128, 128, [T] * 4, 71)
    sn = _pack(dev, ("snake", 128, 128, 3), frag32=True)
    lin = _pack(dev, ("lin", 128, 128, 1))
    assert lin.fx3 is not None
    E = L.EINVAL
    # lengths on the FLAT linears (mrfx_lin, conv_x3 FLAT)
    for form in ("fx3", "x3"):
        for mode in (0, 1):
            _conv(lib, lin, o, 0, 4, T, 1, 1, form=form, act=L.ACT_NONE, adain=False, lens=ln, mode=mode, want=E)
    # bf16 input with FRAG32X3 / X3, t_lens_rows 1 (no kernel reads the fp32 buffer: refused first)
    for form in ("fx3", "x3"):
        _conv(lib, sn, o, 0, 4, T, 3, 1, form=form, act=L.ACT_SNAKE, lens=ln, mode=1, want=E, over=dict(in_dtype=L.BF16))
    # stride != 1 with t_lens_rows 0
    blk = _pack(dev, ("blk", 256, 128, 3), frag32=True)
    ob = Ops(dev, 4, T, 256, 128, [T] * 4, 72)
    for form in ("fx3", "x3"):
        _conv(lib, blk, ob, 0, 4, T, 3, 1, form=form, act=L.ACT_LEAKY, lens=ln, mode=0, want=E,
              over=dict(stride=2, T_out=T // 2))
    # a Snake conv with an accumulate input but no residual (not one of the generator's combinations)
    _conv(lib, sn, o, 0, 4, T, 3, 1, form="fx3", act=L.ACT_SNAKE, acc=True, lens=ln, mode=1, want=E)
    # t_lens_rows 1 with t_lens_mul 2
    for form in ("fx3", "x3"):
        _conv(lib, sn, o, 0, 4, T, 3, 1, form=form, act=L.ACT_SNAKE, lens=ln, mode=1, mul=2, want=E)
    # a Snake conv with t_lens_rows 0, a k7 LeakyReLU conv with lengths (mrfx: no such instance)
    _conv(lib, sn, o, 0, 4, T, 3, 1, form="fx3", act=L.ACT_SNAKE, lens=ln, mode=0, want=E)
    k7 = _pack(dev, ("snake", 128, 128, 7), frag32=True)
    _conv(lib, k7, o, 0, 4, T, 7, 1, form="fx3", act=L.ACT_LEAKY, lens=ln, mode=0, want=E)
