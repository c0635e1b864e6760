"""Conv family: exact staged-operand probes and per-element error bounds (every bf16 conv form on the hot path).

The kernels stage pro(x) as bf16 and feed it to MFMA.  With a one-hot weight (refops.delta_weights), bias 0, no residual
and alpha 1 the output IS the staged operand, bit for bit (every other product is 0 * finite), so one launch per tap
reads the kernel's staged tensor out through every (tile, staged row, tap) pairing, every channel chunk and the
weight-packing permutation.  Each probe launch runs twice: on poisoned, over-allocated, channel-offset operands with
non-compact prologue strides and a NaN-sentinel guarded output, and on compact zero-padded operands; the two must agree
in bits and every guard must be intact.  The dense tests then bound the error of random-weight launches per element
against an fp64 reference evaluated on the staged operands the probe returned.

Figures measured on MI355X stand in each test's docstring.  The bf16 ratios near 1 are the output (or staging) rounding
itself, half an ulp being up to 2^-8 of the value; the fp32-output ratios are small because the accumulation bound is a
worst case over signs.

Mutations of the kernels (scratch builds, each run once on MI355X; "old" = tests/test_gpu_ops.py before this file):
  pro_alpha indexed by ch & 127 in mrfv_body   -> test_probe_snake_mrfv / _wide / _trio (multi-chunk cases: "staged value
                                                  off by 633 of the per-element bound"), test_dense_snake; old: red too
                                                  (the multi-chunk frag32 cases, via lane16 bit-identity and 1.5e-2)
  staging store mask r < rows_in - 1           -> every mrfv probe ("tap 2: zero padding not +0 at ... row 63 of tile 0");
                                                  old: red too
  c_ok = c + 8 <= a.Ci                          -> test_probe_block, Ci 1090 / 130 / 514 ("differs from the exact prologue
                                                  at (0, 0, 1088)"); old: red too (bit-identity with lane16, shortcut)
  bq * a.stat_bs -> bq * a.Ci                   -> 37 mrfv probe / dense tests ("poisoned-layout and compact-layout results
                                                  differ"); old: all 78 conv tests GREEN
  ups_conv: tp <= a.T_final                     -> test_probe_polyphase frag32 / noise, test_dense_polyphase ("a y guard
                                                  was overwritten (rows >= T_final + refl ...)"); old: red in 4 cases
  scalar epilogue stores 8 columns, Co % 8 != 0 -> test_probe_generic (Co 22, ldy 24), test_dense_generic_narrow ("a y
                                                  guard was overwritten"); old: all 17 conv tests GREEN
None faulted."""
import ctypes as C
import math
import os

import pytest
import torch

from refops import (adain_consts, bf, conv_terms_ref, delta_weights, delta_weights_T, dense_ratio, fill_bits, guarded,
                    guards_intact, max_rel, pro_ref64, probe_readout, probe_readout_T, same_bits, staged_check)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 2.0 ** 100                              # finite: 0 * poison = 0
SENT = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FC0A5A5}   # NaN payloads: a write of any value shows
XPADS = (3, 8, 8)   # x: 3 extra rows per utterance, channel offset 8, 8 more columns
YPADS = (2, 8, 8)

# prologues: (AdaIN: None | "p2" (power-of-two sc, sh = 0) | "gen", activation, slope, exact?)
PRO = {
    "none": (None, None, 0.0, True),
    "adain2": ("p2", None, 0.0, True),
    "adain2_leaky8": ("p2", "leaky", 0.125, True),
    "leaky8": (None, "leaky", 0.125, True),
    "leaky.1": (None, "leaky", 0.1, False),
    "leaky.01": (None, "leaky", 0.01, False),
    "adain_leaky.2": ("gen", "leaky", 0.2, False),
    "snake": ("gen", "snake", 0.0, False),
}


@pytest.fixture(scope="module")
def eng(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    yield StyleTTSZS(tiny, tiny_params, device=gpu_device)
    _PROBED.clear()  # (the module's caches go with the module)
    _PACKED.clear()


@pytest.fixture(scope="module")
def ncu(gpu_device):
    return torch.cuda.get_device_properties(gpu_device).multi_processor_count


def _rup(x, m):
    return (x + m - 1) // m * m


class Case:
    """one conv problem: form in lane16 | frag32 | generic | narrow32"""

    def __init__(self, form, B, T, Ci, Co, k, dil=1, stride=1, pad=None, flags=0, in_dt=torch.bfloat16,
                 out_dt=torch.bfloat16, ypads=YPADS):
        self.form, self.B, self.T, self.Ci, self.Co, self.k, self.dil, self.stride = form, B, T, Ci, Co, k, dil, stride
        self.pad = dil * (k - 1) // 2 if pad is None else pad
        self.flags, self.in_dt, self.out_dt, self.ypads = flags, in_dt, out_dt, ypads
        self.T_out = (T + 2 * self.pad - dil * (k - 1) - 1) // stride + 1
        # the narrow form stores whole 8-column vectors (zeros in [Co, ceil8(Co)), include/stzs.h)
        self.Cw = _rup(Co, 8) if form == "narrow32" else Co

    def key(self):
        return (self.form, self.B, self.T, self.Ci, self.Co, self.k, self.dil, self.stride, self.pad, self.flags,
                self.in_dt, self.out_dt)


# ------------------------------------------------------------------ the launcher's form rules, restated
def mrfv_form(ncu, c, pro_act, flags):
    """csrc/mrfv.hip snake_form and the block-conv rules -> (family, chunks, tile form)"""
    from stzs import _lib as L
    ci_pad, co_pad = _rup(c.Ci, 128), _rup(c.Co, 128)
    tiles = c.B * ((c.T_out + 127) // 128)
    wide_tiles, tiles128 = tiles * (co_pad // 256), tiles * (co_pad // 128)
    t128, narrow = bool(flags & L.CONV_MRFV_T128), bool(flags & L.CONV_MRFV_NARROW)
    if pro_act == "snake":
        wide = ci_pad > 128 and co_pad % 256 == 0 and wide_tiles >= 512 and not narrow
        sb64 = {3: 5, 7: 6, 11: 8}[c.k]
        t64 = not wide and tiles128 < 2 * ncu and 64 + (c.k - 1) * c.dil <= 16 * sb64 and not t128
        return "snake", "single" if ci_pad == 128 else "multi", "wide" if wide else "t64" if t64 else "t128"
    wide = ci_pad > 128 and co_pad % 256 == 0 and wide_tiles >= 2 * ncu and not narrow
    t64 = not wide and tiles128 < 4 * ncu and not t128
    return "block", "multi" if ci_pad > 128 else "single", "wide" if wide else "t64" if t64 else "t128"


# ------------------------------------------------------------------ operands
def make_ops(c, pro, seed):
    """host operands of (case, prologue): x, AdaIN statistics / gamma / beta (distinct per utterance), alpha"""
    adain, act, slope, _ = PRO[pro]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(c.B, c.T, c.Ci, generator=g)
    if c.in_dt == torch.bfloat16:
        x = bf(x)
    o = dict(x=x, mean=None, alpha=None)
    if adain == "p2":
        o["mean"] = torch.zeros(c.B, c.Ci)
        o["rstd"] = 2.0 ** torch.randint(-2, 3, (c.B, c.Ci), generator=g).float()
        o["gamma"] = torch.tensor([0.0, 1.0, 3.0, -0.5])[torch.randint(0, 4, (c.B, c.Ci), generator=g)]
        o["beta"] = torch.zeros(c.B, c.Ci)
    elif adain == "gen":
        o["mean"] = torch.randn(c.B, c.Ci, generator=g) * 0.1
        o["rstd"] = torch.rand(c.B, c.Ci, generator=g) + 0.5
        o["gamma"] = torch.randn(c.B, c.Ci, generator=g) * 0.2
        o["beta"] = torch.randn(c.B, c.Ci, generator=g) * 0.2
    if act == "snake":
        o["alpha"] = torch.exp(torch.empty(c.Ci).uniform_(math.log(0.25), math.log(4.0), generator=g))
    return o


def layout(c, o, poisoned):
    """device operands: poisoned = channel-offset x in a wider, longer buffer, statistics / gamma-beta rows with
    non-compact strides, finite poison everywhere else; else compact and zero padded"""
    Ci = c.Ci
    xb, xa = guarded((c.B, c.T, Ci), XPADS if poisoned else (0, 0, 0), POISON if poisoned else 0.0, c.in_dt, DEV)
    xa.t[:, :, xa.c0:xa.c0 + Ci] = o["x"].to(DEV, c.in_dt)
    d = dict(x=xa, xb=xb, pro=None, alpha=o["alpha"].to(DEV) if o["alpha"] is not None else None)
    if o["mean"] is not None:
        sbs, gbs, boff = (Ci + 24, 2 * Ci + 40, Ci + 16) if poisoned else (Ci, 2 * Ci, Ci)
        fill = POISON if poisoned else 0.0
        mean, rstd = (torch.full((c.B, sbs), fill, device=DEV) for _ in range(2))
        gb = torch.full((c.B, gbs), fill, device=DEV)
        mean[:, :Ci], rstd[:, :Ci] = o["mean"].to(DEV), o["rstd"].to(DEV)
        gb[:, :Ci], gb[:, boff:boff + Ci] = o["gamma"].to(DEV), o["beta"].to(DEV)
        d["pro"] = (mean, rstd, sbs, gb.data_ptr(), gbs, boff)
        d["keep"] = gb
    return d


_PACKED = {}


def pack(c, w, b, key=None, ups=0):
    """pack (and cache, for the delta weights) w for the case's form"""
    if key is not None and key in _PACKED:
        return _PACKED[key]
    from stzs.weights import Arena, pack_conv
    A = Arena()
    cw = pack_conv(A, "t", w, b, ups=ups, lane16=c.form == "lane16", frag32=c.form == "frag32",
                   narrow32=c.form == "narrow32")
    A.finalize(DEV)
    cw.w = A[cw.w]
    cw.b = A[cw.b] if cw.b is not None else None
    cw._arena = A
    if key is not None:
        _PACKED[key] = cw
    return cw


def conv_args(eng, c, cw, d, y, pro, **kw):
    """the stzs_conv_args of one launch, as the engine fills and routes them"""
    from stzs import _lib as L
    _, act, slope, _ = PRO[pro]
    grp = []
    eng.conv(cw, d["x"], y, pad=c.pad, dil=c.dil, stride=c.stride, pro=d["pro"],
             pro_act={None: L.ACT_NONE, "leaky": L.ACT_LEAKY, "snake": L.ACT_SNAKE}[act], pro_slope=slope,
             pro_alpha=d["alpha"], flags=c.flags, collect=grp, **kw)
    return grp[0]


def launch(eng, a):
    rc = eng.lib.stzs_conv1d(C.byref(a), eng.stream())
    assert rc == 0, f"stzs_conv1d returned {rc}"


def y_pair(c, B=None, T_out=None, Co=None, ypads=None):
    """(guarded sentinel-filled output, compact zero output) as (buffer, Act) pairs"""
    shp = (c.B if B is None else B, c.T_out if T_out is None else T_out, c.Co if Co is None else Co)
    return (guarded(shp, c.ypads if ypads is None else ypads, SENT[c.out_dt], c.out_dt, DEV),
            guarded(shp, (0, 0, 0), 0.0, c.out_dt, DEV))


def y_intact(yb, ya, C=None):
    """the sentinel around a y_pair output is untouched"""
    return guards_intact(yb, ya, SENT[yb.dtype], C)


def staged_ref(c, o, pro):
    """pro_ref64 of the case's operands, on the device"""
    adain, act, slope, _ = PRO[pro]
    sc = sh = None
    if adain:
        sc, sh = adain_consts(*(o[n].to(DEV) for n in ("mean", "rstd", "gamma", "beta")))
    return pro_ref64(o["x"].to(DEV), sc, sh, act, slope, o["alpha"].to(DEV) if o["alpha"] is not None else None)


_PROBED = {}


def check_staged(S, c, o, pro, label):
    """assertion 1 / 2 on the staged tensor the probe read"""
    s, sbf, mag = staged_ref(c, o, pro)
    got = S if S.dtype == torch.bfloat16 else S.to(torch.bfloat16)
    if S.dtype != torch.bfloat16:
        assert torch.equal(got.float(), S), "an fp32 output of delta weights is not a bf16 value"
    if PRO[pro][3]:
        bad = got.view(torch.int16) != sbf.view(torch.int16)
        assert not bad.any(), (f"{label}: staged value differs from the exact prologue at (utterance, row, channel) "
                               f"{tuple(int(v) for v in bad.nonzero()[0])}: {bad.sum().item()} elements")
    else:
        ratio, share = staged_check(got, s, sbf, mag)
        print(f"{label}: staged max ratio {ratio:.4f}, share of bits differing from bf16(fp64) {share:.3e}")
        assert ratio <= 1, f"{label}: staged value off by {ratio:.3f} of the per-element bound"
        assert share <= 0.01, f"{label}: {share:.4f} of the staged values differ from bf16(fp64)"


def probe(eng, c, pro, seed=0):
    """the staged operand of (case, prologue), read through every tap and channel block on the poisoned layout; every
    launch repeated on the compact layout (same bits) with the output guards checked.  Asserts 1-5; -> (S, operands).
    S and the host operands of the small-batch cases are kept for the tests that reuse them (the device buffers never,
    the wide B = 171 / 256 cases not at all)."""
    k0 = (c.key(), pro, seed)
    if k0 in _PROBED:
        return _PROBED[k0]
    o = make_ops(c, pro, seed)
    dp, dc = layout(c, o, True), layout(c, o, False)
    label = f"{c.form} B{c.B} T{c.T} {c.Ci}->{c.Co} k{c.k} d{c.dil} s{c.stride} {pro} flags {c.flags}"
    problems = []

    def run(j0, m):
        cw = pack(c, delta_weights(c.Co, c.Ci, c.k, j0, m), None, key=(c.form, c.Co, c.Ci, c.k, j0, m))
        (yb, ya), (_, yc) = y_pair(c)
        launch(eng, conv_args(eng, c, cw, dp, ya, pro))
        launch(eng, conv_args(eng, c, cw, dc, yc, pro))
        torch.cuda.synchronize()
        if not y_intact(yb, ya, c.Cw):
            problems.append(f"tap {j0} block {m}: a y guard was overwritten")
        got = ya.t[:, :, ya.c0:ya.c0 + c.Co].clone()
        if not same_bits(got, yc.t[:, :, :c.Co]):
            problems.append(f"tap {j0} block {m}: poisoned-layout and compact-layout results differ")
        if c.Cw > c.Co and bool((ya.t[:, :, ya.c0 + c.Co:ya.c0 + c.Cw] != 0).any()):
            problems.append(f"tap {j0} block {m}: columns [Co, ceil8(Co)) not zero")
        return got

    S, pr = probe_readout(run, T=c.T, Ci=c.Ci, Co=c.Co, k=c.k, dil=c.dil, pad=c.pad, stride=c.stride)
    assert not (problems + pr), label + ": " + "; ".join((problems + pr)[:6])
    assert same_bits(dp["xb"][:, c.T:], fill_bits(dp["xb"][:, c.T:].shape, c.in_dt, POISON, DEV))  # (x is read-only)
    check_staged(S, c, o, pro, label)
    if c.B <= 2:
        _PROBED[k0] = (S, o)
    return S, o


# ------------------------------------------------------------------ §2 probes: Snake forms
SNAKE_SINGLE = [(128, 128, 3, 1), (128, 128, 3, 5), (128, 128, 7, 3), (128, 128, 11, 5)]
SNAKE_MULTI = [(256, 256, 7, 3), (384, 176, 11, 5), (256, 256, 3, 1)]
T64, T128 = (5, 64, 65, 200), (5, 128, 129, 300)


@pytest.mark.parametrize("tile", ["t64", "t128"])
@pytest.mark.parametrize("shape", SNAKE_SINGLE + SNAKE_MULTI)
def test_probe_snake_mrfv(eng, ncu, shape, tile):
    """register-direct Snake forms, single- and multi-chunk, 64-row tiles (the small-grid default) and 128-row tiles
    (STZS_CONV_MRFV_T128), B = 2, T = 5 (shorter than the padding) .. 200 / 300 (an interior tile for every k).
    MI355X: largest staged ratio (|got - s| over 2^-8 |s| + 2^-16 magnitude) 0.9915, share of staged bits differing
    from bf16(fp64) <= 1.9e-4."""
    from stzs import _lib as L
    Ci, Co, k, dil = shape
    for T in (T64 if tile == "t64" else T128):
        c = Case("frag32", 2, T, Ci, Co, k, dil, flags=0 if tile == "t64" else L.CONV_MRFV_T128)
        assert mrfv_form(ncu, c, "snake", c.flags) == ("snake", "single" if Ci == 128 else "multi", tile)
        probe(eng, c, "snake")


@pytest.mark.parametrize("shape", [(256, 256, 3, 1), (256, 256, 11, 5)])
def test_probe_snake_wide(eng, ncu, shape):
    """the wide Snake form (256 output channels per workgroup): B = 171, T = 300 is 513 wide tiles; whole tensor.
    MI355X: staged ratio 0.9922, share 6.9e-5."""
    Ci, Co, k, dil = shape
    c = Case("frag32", 171, 300, Ci, Co, k, dil)
    assert mrfv_form(ncu, c, "snake", 0) == ("snake", "multi", "wide")
    probe(eng, c, "snake")


@pytest.mark.parametrize("shape", SNAKE_SINGLE + SNAKE_MULTI)
def test_probe_snake_lane16(eng, shape):
    """the LDS-ring kernel (csrc/mrf.hip) on every Snake shape above.  The kernel has 128-row tiles only, so it runs the
    128-row T set (5, 128, 129, 300), whose edges are its tile edges; the 64-row set would add no path.  MI355X: staged
    ratio 0.9915, share <= 1.3e-4 -- and the same staged bits as the register-direct forms (asserted)."""
    Ci, Co, k, dil = shape
    for T in T128:
        S, _ = probe(eng, Case("lane16", 2, T, Ci, Co, k, dil), "snake")
        from stzs import _lib as L
        Sv, _ = probe(eng, Case("frag32", 2, T, Ci, Co, k, dil, flags=L.CONV_MRFV_T128), "snake")
        assert same_bits(S, Sv)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("B,T,Cc", [(B, T, Cc) for B in (1, 2) for T in (77, 200) for Cc in (128, 256)])
def test_probe_trio(eng, ncu, B, T, Cc, res):
    """stzs_conv1d_group on delta-weight k3 / k7 / k11 convs (one launch: it returns 1), with and without a residual
    (zeros inside a poisoned buffer, so the sum stays exact): each conv's staged tensor read through all its taps.
    MI355X: staged ratio 0.9875, share <= 7.9e-5."""
    from stzs import _lib as L
    dils = {3: 1, 7: 3, 11: 5}
    cs = {k: Case("frag32", B, T, Cc, Cc, k, dils[k]) for k in (3, 7, 11)}
    o = make_ops(cs[3], "snake", 5)
    dp = layout(cs[3], o, True)
    rb, ra = guarded((B, T, Cc), XPADS, POISON, torch.bfloat16, DEV)
    ra.t[:, :, ra.c0:ra.c0 + Cc] = 0
    ys = {k: {} for k in cs}
    problems = []
    for jj in range(11):
        args, outs = [], []
        for k, c in cs.items():
            assert mrfv_form(ncu, c, "snake", 0)[2] == "t64"
            j0 = jj % k
            cw = pack(c, delta_weights(Cc, Cc, k, j0), None, key=("frag32", Cc, Cc, k, j0, 0))
            (yb, ya), _ = y_pair(c)
            args.append(conv_args(eng, c, cw, dp, ya, "snake", res=ra if res else None))
            outs.append((k, j0, yb, ya))
        n = eng.lib.stzs_conv1d_group((L.ConvArgs * 3)(*args), 3, eng.stream())
        assert n == 1, n
        torch.cuda.synchronize()
        for k, j0, yb, ya in outs:
            if not y_intact(yb, ya):
                problems.append(f"k{k} tap {j0}: a y guard was overwritten")
            ys[k][j0] = ya.t[:, :, ya.c0:ya.c0 + Cc].clone()
    for k, c in cs.items():
        S, pr = probe_readout(lambda j0, m: ys[k][j0], T=T, Ci=Cc, Co=Cc, k=k, dil=c.dil, pad=c.pad)
        assert not (problems + pr), f"trio k{k}: " + "; ".join((problems + pr)[:6])
        check_staged(S, c, o, "snake", f"trio B{B} T{T} C{Cc} k{k} res {res}")
        if not res:  # the same bits as the conv alone
            assert same_bits(S, probe(eng, c, "snake", 5)[0])


# ------------------------------------------------------------------ §2 probes: block convs
BLOCKS = [(1090, 256, 3, "adain2_leaky8"), (1090, 256, 3, "adain_leaky.2"), (130, 64, 3, "none"), (130, 64, 3, "adain2"),
          (200, 96, 3, "adain2_leaky8"), (200, 96, 3, "adain_leaky.2"), (514, 256, 3, "adain2_leaky8"),
          (514, 256, 3, "none"), (1090, 256, 1, "none"), (514, 256, 1, "none"), (130, 64, 1, "none")]


# (the wide form needs co_pad % 256 == 0: the narrower shapes have no such form)
BLOCK_CASES = [b + (t,) for b in BLOCKS for t in ("t64", "t128", "wide") if t != "wide" or b[1] == 256]


@pytest.mark.parametrize("Ci,Co,k,pro,tile", BLOCK_CASES)
def test_probe_block(eng, ncu, Ci, Co, k, pro, tile):
    """the LeakyReLU / identity block convs and their 1x1 shortcut on the register-direct forms: 64-row tiles, 128-row
    tiles (STZS_CONV_MRFV_T128), and the wide form at B = 256, T = 130, Co = 256 (the second tile has 2 valid rows).
    1090 channels: 9 chunks, the last vector holds 2 real channels.  MI355X (AdaIN + LeakyReLU(0.2)): staged ratio
    0.9922, share <= 7.7e-5."""
    from stzs import _lib as L
    if tile == "wide":
        c = Case("frag32", 256, 130, Ci, Co, k)
    else:
        c = Case("frag32", 2, 130, Ci, Co, k, flags=0 if tile == "t64" else L.CONV_MRFV_T128)
    assert mrfv_form(ncu, c, PRO[pro][1], c.flags)[::2] == ("block", tile)
    probe(eng, c, pro)


# ------------------------------------------------------------------ §2 probes: generic conv_mfma, narrow conv
GENERIC = [
    (dict(Ci=22, Co=32, k=12, stride=6, pad=3, T=385), ("none", "adain2_leaky8", "snake")),   # the stride-6 noise conv
    (dict(Ci=96, Co=80, k=3, T=129), ("none", "adain2_leaky8", "snake", "adain_leaky.2")),
    (dict(Ci=96, Co=80, k=3, T=5), ("adain2_leaky8",)),
    (dict(Ci=64, Co=22, k=3, T=129, ypads=(2, 0, 0)), ("none", "adain2_leaky8")),            # ldy 24: scalar epilogue
    (dict(Ci=96, Co=80, k=3, T=129, in_dt=torch.float32, out_dt=torch.float32), ("none", "adain2_leaky8", "snake")),
]


@pytest.mark.parametrize("kw,pros", GENERIC)
def test_probe_generic(eng, kw, pros):
    """the generic conv_mfma path: strided, Ci / Co below a tile, the scalar epilogue (Co % 8 != 0, ldy = 24), fp32 in
    and out (the staged value is then the one rounding of the fp32 prologue value to bf16).  MI355X (Snake by the
    hardware sine): staged ratio 0.9865, share 8.1e-5; AdaIN + LeakyReLU(0.2): 0.9917, 0."""
    from stzs.engine import _conv_generic
    for pro in pros:
        c = Case("generic", 2, **kw)
        S, o = probe(eng, c, pro)
        cw = pack(c, delta_weights(c.Co, c.Ci, c.k, 0, 0), None, key=(c.form, c.Co, c.Ci, c.k, 0, 0))
        a = conv_args(eng, c, cw, layout(c, o, True), y_pair(c)[0][1], pro)
        assert _conv_generic(a.flags, cw), a.flags


@pytest.mark.parametrize("Co", [8, 22, 32])
@pytest.mark.parametrize("k", [3, 7])
def test_probe_narrow(eng, Co, k):
    """the narrow conv (conv_post form, fp32 out, 256-row tiles): T = 5 .. 257.  MI355X (LeakyReLU(0.01)): staged ratio
    0.667, share 0."""
    for T in (5, 127, 129, 257):
        for pro in ("none", "leaky8", "leaky.01") if T == 257 else ("leaky8",):
            probe(eng, Case("narrow32", 2, T, 128 if k == 7 else 256, Co, k, out_dt=torch.float32), pro)


# ------------------------------------------------------------------ §2 probes: polyphase ConvTranspose
UPS = [(s, refl, Ci) for s in (4, 6, 10) for refl in (0, 1) for Ci in (128, 200, 512)]


def ups_rows(Ci):
    """csrc/ups.hip stzs_ups_conv_launch: 64-row q tiles where more than two 128-channel chunks are staged, else 128
    (STZS_UPS_BT, read once per process, would override it: the tests need it unset)"""
    assert os.environ.get("STZS_UPS_BT") is None
    return 64 if _rup(Ci, 128) // 128 > 2 else 128


def _ups_run(eng, packing, B, T, Ci, Co, s, refl, pro, seed=0):
    """probe the polyphase form -> (S, problems, operands, layout)"""
    from stzs import _lib as L
    from stzs.weights import Arena, pack_ups_noise
    c = Case("lane16" if packing == "lane16" else "frag32", B, T, Ci, Co, 2 * s)
    _, act, slope, _ = PRO[pro]
    o = make_ops(c, pro, seed)
    dp, dc = layout(c, o, True), layout(c, o, False)
    Tn, pad = T * s + refl, s // 2
    kw = dict(pro_act=L.ACT_LEAKY if act else L.ACT_NONE, pro_slope=slope, ups_pad=pad, T_final=T * s, refl=refl)
    har = None
    if packing == "noise":
        har = guarded((B, Tn, 32), XPADS, POISON, torch.bfloat16, DEV)[1]
        har.t[:, :, har.c0:har.c0 + 32] = 0
        har.t[:, :, har.c0:har.c0 + 22] = torch.randn(B, Tn, 22, generator=torch.Generator().manual_seed(T)).to(
            DEV, torch.bfloat16)
    problems = []

    def run(j0, m):
        key = (packing, "ups", Co, Ci, s, j0, m)
        w = delta_weights_T(Ci, Co, 2 * s, j0, m)
        if packing == "noise":
            if key not in _PACKED:
                A = Arena()
                cw = pack_ups_noise(A, "t", w, torch.zeros(Co), torch.zeros(Co, 22, 1), torch.zeros(Co))
                A.finalize(DEV)
                cw.w, cw.b, cw.nz32, cw._arena = A[cw.w], A[cw.b], A[cw.nz32], A
                _PACKED[key] = cw
            cw = _PACKED[key]
            extra = dict(res=har, flags=L.CONV_UPS_NOISE, gate=cw.nz32.data_ptr())
        else:
            cw, extra = pack(c, w, None, key=key, ups=s), {}
        (yb, ya), (_, yc) = y_pair(c, T_out=Tn)
        for d, y in ((dp, ya), (dc, yc)):
            eng.conv(cw, d["x"], y, **kw, **extra)
        torch.cuda.synchronize()
        if not y_intact(yb, ya):
            problems.append(f"tap {j0} block {m}: a y guard was overwritten (rows >= T_final + refl included)")
        got = ya.t[:, :, ya.c0:ya.c0 + Co].clone()
        if not same_bits(got, yc.t[:, :, :Co]):
            problems.append(f"tap {j0} block {m}: poisoned-layout and compact-layout results differ")
        return got

    S, pr = probe_readout_T(run, T=T, Ci=Ci, Co=Co, ups=s, ups_pad=pad, refl=refl)
    return S, problems + pr, c, o


@pytest.mark.parametrize("packing", ["lane16", "frag32", "noise"])
@pytest.mark.parametrize("s,refl,Ci", UPS)
def test_probe_polyphase(eng, packing, s, refl, Ci):
    """the polyphase ConvTranspose -- LANE16 (csrc/mrf.hip), FRAG32 (csrc/ups.hip: 128-row tiles, 64-row tiles at Ci =
    512) and the fused noise conv with a zero noise weight -- at input T = 1 .. 129: every output row equals
    leaky(x)[q] at t = q s + p - pad + refl, row 0 mirrors row 2's source, every other row is +0, and nothing is written
    at t >= T_final + refl.  MI355X (LeakyReLU(0.1)): staged ratio 0.7604, share 0."""
    Co = 256 if Ci == 512 else 128
    assert ups_rows(Ci) == (64 if Ci == 512 else 128)  # (the tile height the docstring labels the case with)
    for T in (1, 2, 64, 65, 129):
        for pro in ("none", "leaky8", "leaky.1") if T == 65 else ("leaky8",):
            S, problems, c, o = _ups_run(eng, packing, 2, T, Ci, Co, s, refl, pro)
            label = f"ups {packing} s{s} refl{refl} T{T} {Ci}->{Co} {pro}"
            assert not problems, label + ": " + "; ".join(problems[:6])
            check_staged(S, c, o, pro, label)


# ------------------------------------------------------------------ §3 dense per-element bounds
def dense_prep(eng, c, pro, *, res=False, tdiv=1, acc=False, alpha=1.0, stat=False, utts=None, label="", seed=0):
    """a dense problem: random weights / bias / residual / accumulate input (+ fused statistics with stat_ld > Co) on the
    poisoned layout -> (its stzs_conv_args, the check to run after the launch: dense_check)"""
    S, o = probe(eng, c, pro, seed)
    dp = layout(c, o, True)
    g = torch.Generator().manual_seed(c.Ci + c.k + c.T)
    w = bf(torch.randn(c.Co, c.Ci, c.k, generator=g) / math.sqrt(c.Ci * c.k))
    b = torch.randn(c.Co, generator=g) * 0.1
    cw = pack(c, w, b)
    rnd = lambda T: torch.randn(c.B, T, c.Co, generator=g).to(c.out_dt)
    r_h = rnd((c.T_out + tdiv - 1) // tdiv) if res else None
    a_h = rnd(c.T_out) if acc else None

    def dev_act(h):
        if h is None:
            return None
        _, a = guarded(tuple(h.shape), YPADS, POISON, c.out_dt, DEV)
        a.t[:, :, a.c0:a.c0 + c.Co] = h.to(DEV)
        return a
    rd, ad = dev_act(r_h), dev_act(a_h)
    (yb, ya), _ = y_pair(c)
    a = conv_args(eng, c, cw, dp, ya, pro, res=rd, res_tdiv=tdiv, acc_in=ad, alpha=alpha, beta=0.5 if acc else 0.0)
    slab = None
    if stat:
        nch, sld = (c.T_out + 63) // 64, _rup(c.Co, 8) + 8
        slab = fill_bits((c.B, nch, sld, 2), torch.float32, SENT[torch.float32], DEV)
        a.stat_part, a.stat_ld = slab.data_ptr(), sld
    keep = (cw, dp, rd, ad)  # (alive until the check has run)
    return a, lambda: dense_check(c, S, w, b, r_h, a_h, tdiv, alpha, acc, slab, yb, ya, utts, label, keep)


def dense_check(c, S, w, b, r_h, a_h, tdiv, alpha, acc, slab, yb, ya, utts, label, keep):
    """the launched dense problem against the fp64 reference on the staged operands the probe returned -> the largest
    ratio to the per-element bound (asserted <= 1); fused statistics by the 1e-5 rule"""
    assert y_intact(yb, ya, c.Cw), label + ": a y guard was overwritten"
    got = ya.t[:, :, ya.c0:ya.c0 + c.Co].cpu()
    ub = list(range(c.B)) if utts is None else utts
    sel = lambda t: t[ub] if t is not None else None
    ref, terms = conv_terms_ref(S[ub].float().cpu(), w, b, pad=c.pad, dil=c.dil, stride=c.stride, res=sel(r_h),
                                res_tdiv=tdiv, out_scale=alpha, acc_in=sel(a_h), beta=0.5 if acc else 0.0)
    ratio = dense_ratio(got[ub], ref, terms, c.Ci * c.k, c.out_dt == torch.bfloat16)
    print(f"{label}: dense max ratio {ratio:.4f}")
    assert ratio <= 1, f"{label}: {ratio:.3f} of the per-element bound"
    if slab is not None:  # the existing rule: statistics within 1e-5 of those of the stored tensor
        part = slab[:, :, :c.Co].double().cpu()
        assert same_bits(slab[:, :, c.Co:], fill_bits(slab[:, :, c.Co:].shape, torch.float32, SENT[torch.float32], DEV))
        y = got.double()
        m = part[..., 0].sum(1) / c.T_out
        v = (part[..., 1].sum(1) / c.T_out - m * m).clamp_min(0)
        mr, vr = y.mean(1), y.var(1, unbiased=False)
        assert float(((m - mr).abs() / (mr.abs() + vr.sqrt())).max()) < 1e-5
        assert max_rel(1 / torch.sqrt(v + 1e-5), 1 / torch.sqrt(vr + 1e-5)) < 1e-5
    return ratio


def dense(eng, c, pro, **kw):
    """one dense problem, launched alone -> the largest ratio to the bound"""
    a, check = dense_prep(eng, c, pro, **kw)
    launch(eng, a)
    torch.cuda.synchronize()
    return check()


def test_dense_snake(eng):
    """Snake forms with residual, alpha, accumulate input and fused statistics.  MI355X largest ratio: single chunk
    0.87 (64-row), 0.96 (128-row), multi-chunk 0.46 (64-row), 0.76 (128-row), LDS ring 0.76, wide (utterances 0, 85,
    170) 0.70."""
    from stzs import _lib as L
    dense(eng, Case("frag32", 2, 200, 128, 128, 11, 5), "snake", res=True, acc=True, alpha=1 / 3, label="snake single t64")
    dense(eng, Case("frag32", 2, 300, 128, 128, 3, 5, flags=L.CONV_MRFV_T128), "snake", res=True, stat=True,
          alpha=0.7071, label="snake single t128")
    dense(eng, Case("frag32", 2, 200, 384, 176, 11, 5), "snake", res=True, stat=True, alpha=0.7071, label="snake multi t64")
    dense(eng, Case("frag32", 2, 300, 256, 256, 7, 3, flags=L.CONV_MRFV_T128), "snake", res=True, acc=True, stat=True,
          alpha=1 / 3, label="snake multi t128")
    dense(eng, Case("lane16", 2, 300, 256, 256, 7, 3), "snake", res=True, acc=True, stat=True, alpha=1 / 3,
          label="snake lane16")
    dense(eng, Case("frag32", 171, 300, 256, 256, 11, 5), "snake", res=True, acc=True, stat=True, alpha=1 / 3,
          utts=[0, 85, 170], label="snake wide")


@pytest.mark.parametrize("B,T,Cc", [(2, 200, 256), (1, 77, 128)])
def test_dense_trio(eng, ncu, B, T, Cc):
    """stzs_conv1d_group on dense k3 / k7 / k11 convs of one input (residual, fused statistics with stat_ld > Co; alpha 1
    and no accumulate input, as the one-launch form requires): it returns 1, and every conv meets the per-element bound
    against its own probed staged operand (test_probe_trio: the trio stages the same bits).  MI355X largest ratio:
    k3 0.92, k7 0.84, k11 0.74."""
    from stzs import _lib as L
    dils = {3: 1, 7: 3, 11: 5}
    preps = []
    for k in (3, 7, 11):
        c = Case("frag32", B, T, Cc, Cc, k, dils[k])
        assert mrfv_form(ncu, c, "snake", 0)[2] == "t64"
        preps.append(dense_prep(eng, c, "snake", res=True, stat=True, label=f"trio B{B} T{T} C{Cc} k{k}", seed=5))
    n = eng.lib.stzs_conv1d_group((L.ConvArgs * 3)(*(a for a, _ in preps)), 3, eng.stream())
    assert n == 1, n
    torch.cuda.synchronize()
    for _, check in preps:
        check()


def test_dense_block(eng):
    """block convs with the x2 shortcut residual (res_tdiv = 2) and fused statistics.  MI355X largest ratio: 1090->256
    0.56 (64-row), 0.56 (128-row), 0.54 (wide, utterances 0, 128, 255); 200->96 0.90; shortcut 0.83."""
    from stzs import _lib as L
    for fl, lab in ((0, "t64"), (L.CONV_MRFV_T128, "t128")):
        dense(eng, Case("frag32", 2, 130, 1090, 256, 3, flags=fl), "adain_leaky.2", res=True, tdiv=2, stat=True,
              alpha=0.7071, label="block 1090->256 " + lab)
    dense(eng, Case("frag32", 256, 130, 1090, 256, 3), "adain_leaky.2", res=True, tdiv=2, stat=True, alpha=0.7071,
          utts=[0, 128, 255], label="block 1090->256 wide")
    dense(eng, Case("frag32", 2, 130, 200, 96, 3), "adain_leaky.2", stat=True, label="block 200->96")
    dense(eng, Case("frag32", 2, 130, 1090, 256, 1), "none", label="shortcut 1090->256")


def test_dense_generic_narrow(eng):
    """the generic conv (strided; fp32 in / out: the 2 (K + 4) 2^-24 bound alone; scalar epilogue) and the narrow conv.
    MI355X largest ratio: stride-6 0.93, 96->80 bf16 0.95, fp32 0.0024, Co 22 0.97, narrow 0.0010."""
    dense(eng, Case("generic", 2, 385, 22, 32, 12, stride=6, pad=3), "snake", res=True, acc=True, alpha=1 / 3,
          label="generic stride 6")
    dense(eng, Case("generic", 2, 129, 96, 80, 3), "snake", res=True, stat=True, alpha=0.7071, label="generic 96->80")
    dense(eng, Case("generic", 2, 129, 96, 80, 3, in_dt=torch.float32, out_dt=torch.float32), "snake", res=True,
          acc=True, stat=True, alpha=1 / 3, label="generic fp32")
    dense(eng, Case("generic", 2, 129, 64, 22, 3, ypads=(2, 0, 0)), "adain2_leaky8", alpha=0.5, label="generic Co 22")
    dense(eng, Case("narrow32", 2, 257, 128, 22, 7, out_dt=torch.float32), "leaky.01", alpha=0.5, label="narrow")


@pytest.mark.parametrize("packing", ["lane16", "frag32"])
def test_dense_polyphase(eng, packing):
    """the polyphase ConvTranspose with a residual, dense weights (K = 2 Ci per output).  MI355X largest ratio 0.89
    (both packings)."""
    from stzs import _lib as L
    B, T, Ci, Co, s, refl = 2, 129, 512, 256, 6, 1
    S, problems, c, o = _ups_run(eng, packing, B, T, Ci, Co, s, refl, "leaky.1")
    assert not problems, problems[:6]
    g = torch.Generator().manual_seed(s)
    w = bf(torch.randn(Ci, Co, 2 * s, generator=g) / math.sqrt(Ci * 2))
    b = torch.randn(Co, generator=g) * 0.1
    Tn = T * s + refl
    r_h = bf(torch.randn(B, Tn, Co, generator=g))
    _, rd = guarded((B, Tn, Co), YPADS, POISON, torch.bfloat16, DEV)
    rd.t[:, :, rd.c0:rd.c0 + Co] = r_h.to(DEV)
    dp = layout(c, o, True)
    (yb, ya), _ = y_pair(c, T_out=Tn)
    eng.conv(pack(c, w, b, ups=s), dp["x"], ya, pro_act=L.ACT_LEAKY, pro_slope=0.1, ups_pad=s // 2, T_final=T * s,
             refl=refl, res=rd)
    torch.cuda.synchronize()
    assert y_intact(yb, ya)
    ref, terms = conv_terms_ref(S.float().cpu(), w, b, ups=s, ups_pad=s // 2, refl=refl, res=r_h)
    ratio = dense_ratio(ya.t[:, :, ya.c0:ya.c0 + Co].cpu(), ref, terms, 2 * Ci, True)
    print(f"polyphase {packing}: dense max ratio {ratio:.4f}")
    assert ratio <= 1


@pytest.mark.parametrize("B,T,Ci,Co,s,refl", [(2, 129, 512, 256, 6, 1), (2, 65, 200, 128, 10, 0)])
def test_dense_polyphase_noise(eng, B, T, Ci, Co, s, refl):
    """the polyphase ConvTranspose with the 1x1 noise conv fused as one more K-step (STZS_CONV_UPS_NOISE), dense weights
    and a nonzero noise conv on poisoned, guarded harmonic-source rows: y = ReflectionPad(convT(S) + bias) + W_noise har
    in fp64 on the probed S, K = 2 Ci + 32, terms = the ConvTranspose's + |W_noise| |har|.  With refl, row 0 is bounded
    too: the kernel forms it as row 2's accumulator (ConvTranspose + W_noise har[2]) plus the fp32 correction
    W_noise (har[0] - har[2]), so its terms are row 2's plus |W_noise| (|har[0]| + |har[2]|) and its K is 32 more.
    MI355X largest ratio: 0.96 (s 10, refl 0), 0.86 (s 6, refl 1), its row 0 0.73."""
    from stzs import _lib as L
    from stzs.weights import Arena, pack_ups_noise
    Ch = 22
    S, problems, c, o = _ups_run(eng, "noise", B, T, Ci, Co, s, refl, "leaky.1")
    assert not problems, problems[:6]
    assert ups_rows(Ci) == (64 if Ci == 512 else 128)
    g = torch.Generator().manual_seed(s + T)
    wu = bf(torch.randn(Ci, Co, 2 * s, generator=g) / math.sqrt(Ci * 2))
    bu = torch.randn(Co, generator=g) * 0.1
    wn = bf(torch.randn(Co, Ch, 1, generator=g) / math.sqrt(Ch))
    bn = torch.randn(Co, generator=g) * 0.1
    Tn = T * s + refl
    h_h = bf(torch.randn(B, Tn, Ch, generator=g))
    _, har = guarded((B, Tn, 32), XPADS, POISON, torch.bfloat16, DEV)
    har.t[:, :, har.c0:har.c0 + 32] = 0          # (channels past the noise conv's input width are zero: the contract)
    har.t[:, :, har.c0:har.c0 + Ch] = h_h.to(DEV)
    A = Arena()
    cw = pack_ups_noise(A, "t", wu, bu, wn, bn)
    A.finalize(DEV)
    cw.w, cw.b, cw.nz32 = A[cw.w], A[cw.b], A[cw.nz32]
    dp = layout(c, o, True)
    (yb, ya), _ = y_pair(c, T_out=Tn)
    eng.conv(cw, dp["x"], ya, pro_act=L.ACT_LEAKY, pro_slope=0.1, ups_pad=s // 2, T_final=T * s, refl=refl, res=har,
             flags=L.CONV_UPS_NOISE, gate=cw.nz32.data_ptr())
    torch.cuda.synchronize()
    assert y_intact(yb, ya)
    got = ya.t[:, :, ya.c0:ya.c0 + Co].cpu()
    # the bias as packed: one fp32 sum of the two
    ref, terms = conv_terms_ref(S.float().cpu(), wu, bu.float() + bn.float(), ups=s, ups_pad=s // 2, refl=refl)
    wd = wn[:, :, 0].double()
    ref = ref + torch.einsum("btj,cj->btc", h_h.double(), wd)
    nmag = torch.einsum("btj,cj->btc", h_h.double().abs(), wd.abs())
    terms = terms + nmag
    K = 2 * Ci + 32
    ratio = dense_ratio(got[:, refl:], ref[:, refl:], terms[:, refl:], K, True)
    print(f"polyphase noise s{s} refl{refl} {Ci}->{Co}: dense max ratio {ratio:.4f}")
    assert ratio <= 1
    if refl:
        t0 = terms[:, 2:3] + nmag[:, 0:1] + nmag[:, 2:3]
        r0 = dense_ratio(got[:, :1], ref[:, :1], t0, K + 32, True)
        print(f"polyphase noise s{s} refl{refl} {Ci}->{Co}: row 0 max ratio {r0:.4f}")
        assert r0 <= 1


@pytest.mark.parametrize("act", ["gelu", "silu"])
def test_dense_flat_gemm_act(eng, act):
    """GELU / SiLU epilogue of the FLAT GEMM, fp32 out (512 -> 384, 6 x 50 rows): 1.13 (the Lipschitz bound of both
    activations) times the accumulation bound, + 4e-7 (1 + |z|) for fast_erf (1.5e-7) and __expf.  MI355X largest
    ratio: GELU 0.0013, SiLU 0.0013."""
    from stzs import _lib as L
    from stzs.engine import Act
    g = torch.Generator().manual_seed(11)
    R, Lr, Ci, Co = 6, 50, 512, 384
    x = bf(torch.randn(R, Lr, Ci, generator=g))
    w = bf(torch.randn(Co, Ci, generator=g) / math.sqrt(Ci))
    b = torch.randn(Co, generator=g) * 0.1
    c = Case("generic", R, Lr, Ci, Co, 1, out_dt=torch.float32)
    (yb, ya), _ = y_pair(c)
    grp = []
    eng.conv(pack(c, w, b), Act(x.to(DEV, torch.bfloat16)), ya, epi_act=L.ACT_GELU if act == "gelu" else L.ACT_SILU,
             collect=grp)
    assert grp[0].flags & 8 and not grp[0].flags & L.CONV_ROWS, grp[0].flags  # STZS_CONV_A_DMA: the FLAT LDS-DMA GEMM
    launch(eng, grp[0])
    torch.cuda.synchronize()
    assert y_intact(yb, ya)
    z, terms = conv_terms_ref(x, w[:, :, None], b)
    ref = 0.5 * z * (1 + torch.erf(z / math.sqrt(2))) if act == "gelu" else z / (1 + torch.exp(-z))
    bound = 1.13 * 2 * (Ci + 4) * 2.0 ** -24 * terms + 4e-7 * (1 + z.abs())
    ratio = ((ya.t[:, :, ya.c0:ya.c0 + Co].cpu().double() - ref).abs() / bound).max().item()
    print(f"flat GEMM {act}: max ratio {ratio:.4f}")
    assert ratio <= 1
