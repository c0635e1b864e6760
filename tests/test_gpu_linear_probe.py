"""The linears: exact operand probes and per-element error bounds for gemm_glds (csrc/gemm.hip), gemm_rows
(csrc/rows.hip), rows16 and ln_rows (csrc/lnrows.hip) -- the four kernels the whole denoiser and every per-utterance
linear run on.

A. Identity probes.  With a one-hot weight (refops.delta_weights, one tap), bias 0 and no epilogue operands the output
   IS the kernel's staged A operand bit for bit, through split-K, the wave-partial sums and the fp8 dequantisation
   (every partial is 0 + x).  Each case (refops.linear_cases: axis sweeps over K-step counts, row counts, widths,
   dtypes, slices) runs on a poisoned, channel-offset, non-compact layout (bsx != T ldx, bsy != T ldy) with a
   NaN-sentinel guarded output and on the compact zero-padded layout: y[:, :, :Ci] has x's bits, columns [Ci, Co) are
   +0, both layouts agree in bits, every y guard is intact, x and its guards are unchanged, the split forms leave
   their counters zero and repeat their bits on them, and stay inside a workspace sized exactly by the library.
   Every case asserts its form first (refops.lin_launch: flags, splitk, entry point); the grids are checked without a
   device in tests/test_dispatch_trace.py on the same table.
B. Dense launches with random weights on the poisoned layout against an fp64 reference, per element: refops.dense_ratio
   with K = ci_pad + extra (extra = fp32 roundings beyond the K chain: 3 for gemm_rows' four wave partials, Z - 1 for
   the slices, 2 for the fp8 acc (sx sw)), GELU / SiLU by refops.act_ratio.
C. ln_rows: the operand image (identity weight, fp32 out) against an fp64 LayerNorm by test_row_layernorm_edges' rule,
   then dense launches against fp64 on the image just read.

Figures measured on MI355X stand in each test's docstring.  The bf16 ratios near 1 are the output rounding itself; the
fp32-output ratios are small because the accumulation bound is a worst case over signs.

Mutations of the kernels (scratch builds, value-only, each run once on MI355X against this file and against the five
older files test_gpu_rows / _lnrows / _splitk / _gemm_xcd / _fp8 = "old"):
  gswz constant 0x1320 -> 0x1230 in rows.hip        -> 32 tests, first test_probe_identity[rows-3x43-128to200-Z0-bf16-f32]
                                                        ("the output is not the staged operand (+0 in columns >= Ci): 8247
                                                        elements differ; first at (utterance, row, column) (0, 0, 4)");
                                                        old: red too (34 of test_gpu_rows.py)
  re-copy of K-step NKS - 2 in gemm_glds::fill       -> nothing, here or in old: the re-copied slot is retired, as designed
  sw[nt ^ 1] in the fp8 dequantisation               -> test_dense_glds_fp8 ("19794911.754 of the per-element bound"); the
                                                        identity probes cannot see it (their column scales are all 1);
                                                        old: red too (test_gemm_f8)
  slice sum s = 1 .. SK - 2 in splitk_combine        -> 24 tests, first test_probe_identity[glds-3x43-64to200-Z2-bf16-bf16]
                                                        ("4128 elements differ; first at ... (0, 0, 32): got 0.0, expected
                                                        0.2001953125"); old: red too (test_gpu_splitk, test_gpu_gemm_xcd)
  gate row bdiv(Rc) -> bdiv(r0) in gemm_rows         -> test_dense_small_m[o-rows], [ff2-rows] ("6287.584 of the
                                                        per-element bound"); old: red too (19 of test_gpu_rows.py)
  the scalar gate read gp[min(co + j + 1, Co - 1)]   -> test_dense_glds (the Co 22, ldy 24 case: "3841.656 of the per-element
  of the FLAT epilogue (conv_common.hpp)                bound"); old: all 138 tests GREEN (no linear there takes the scalar
                                                        epilogue)
  x batch stride T_in ldx instead of bsx, gemm_glds  -> 58 tests, first test_probe_identity[glds-3x43-22to200-Z0-bf16-bf16]
                                                        ("poisoned-layout and compact-layout results differ: 1892 elements
                                                        differ; first at ... (1, 0, 0): got 1.2676506002282294e+30"); old:
                                                        all 138 tests GREEN (compact strides only)
None faulted.  Of the five mutations the issue names, none is caught here and by none of the old files (errors of that
size show in a max-norm over random operands; one is value-neutral by design); the last two, which touch only what the
old files never ran -- the scalar epilogue of a linear, a non-compact stride -- are: 2 of 7."""
import math

import pytest
import torch

from refops import (LIN_DT, LIN_PACKED, LIN_POISON, LIN_SENT, LinCase, act_ratio, bf, conv_terms_ref, dense_ratio,
                    e4m3_value, first_diff, gemm_tile_rows, guarded, guards_intact, layernorm_image_ok, layernorm_ref64,
                    lin_ci_pad, lin_id, lin_launch, lin_make_x, lin_onehot, lin_pack, lin_x_layout, lin_y_layout,
                    linear_cases, linear_probe_expect, quant_rows_ref, round_bf16, same_bits, staged_check)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 1 << 14  # fp32 words behind an exactly-sized split-K workspace


@pytest.fixture(scope="module")
def eng(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    yield StyleTTSZS(tiny, tiny_params, device=gpu_device)
    LIN_PACKED.clear()


@pytest.fixture(scope="module")
def ncu(gpu_device):
    return torch.cuda.get_device_properties(gpu_device).multi_processor_count


# ------------------------------------------------------------------ operands (refops.lin_*, on the device)
def pack(c, w, b=None, key=None):
    return lin_pack(c, w, b, key, DEV)


def onehot(c, m):
    return lin_onehot(c, m, DEV)


def x_layout(c, x, poisoned):
    return lin_x_layout(c, x, poisoned, DEV)


def y_layout(c, poisoned):
    return lin_y_layout(c, poisoned, DEV)


def scale_layout(c, sx):
    """x_scale exactly B T long inside a guarded buffer (NaN behind it: a read past the last row poisons the output)"""
    if sx is None:
        return None, None
    buf = torch.full((sx.numel() + 64,), float("nan"), device=DEV)
    buf[:sx.numel()] = sx.to(DEV)
    return buf, buf[:sx.numel()]


class exact_ws:
    """the engine's split-K workspace sized exactly by the library (stzs_conv_splitk_workspace / _rows_workspace) with a
    guard region behind it, and its counters: after the block, `ok()` says the guard is untouched"""

    def __init__(self, eng, c, cw):
        self.eng, self.c = eng, c
        M = c.B * c.T
        self.nb = 0
        if c.Z > 1:
            self.nb = eng.lib.stzs_conv_rows_workspace(M, c.Co, c.Z) if c.kern in ("rows", "rows16") else \
                eng.lib.stzs_conv_splitk_workspace(M, cw.co_pad, c.Z)
            assert self.nb > 0 and self.nb % 16 == 0
        self.store = torch.full((self.nb // 4 + GUARD,), 12345.0, device=DEV)
        self.names = ("rows_ws", "sk_ws")
        self.ctr = "rows_ctr" if c.kern in ("rows", "rows16") else "sk_ctr"

    def __enter__(self):
        self.orig = self.eng._scratch
        self.eng._scratch = lambda name, n, *a, **k: self.store if name.startswith(self.names) else self.orig(name, n, *a, **k)
        return self

    def __exit__(self, *exc):
        self.eng._scratch = self.orig

    def ok(self):
        return bool((self.store[self.nb // 4:] == 12345.0).all())

    def counters_zero(self):
        t = self.eng._bufs.get(self.ctr + self.eng._branch)
        return t is None or int(t.abs().sum()) == 0


# ------------------------------------------------------------------ A. identity probes
def identity(eng, c, seed=0):
    """the staged operand of a case read through every column block on both layouts; asserts 1-6 -> the staged tensor
    [B, T, Ci] in the output dtype (device)"""
    label = lin_id(c)
    x, sx, staged = lin_make_x(c, seed)
    nblk = (c.Ci + c.Co - 1) // c.Co if c.Co < c.Ci else 1
    res = {}
    for poisoned in (True, False):
        xb, xa = x_layout(c, x, poisoned)
        x0 = xb.clone()
        sbuf, sv = scale_layout(c, sx)
        for m in range(nblk):
            cw = onehot(c, m)
            yb, ya = y_layout(c, poisoned)
            with exact_ws(eng, c, cw) as ws:
                lin_launch(eng, c, cw, xa, ya, x_scale=sv)
                torch.cuda.synchronize()
                got = ya.t[:, :, ya.c0:ya.c0 + c.Co].clone()
                if c.Z > 1:
                    assert ws.counters_zero(), f"{label}: a split-K counter is not zero after the launch"
                    yb2, ya2 = y_layout(c, poisoned)
                    lin_launch(eng, c, cw, xa, ya2, x_scale=sv)
                    torch.cuda.synchronize()
                    assert same_bits(ya2.t[:, :, ya2.c0:ya2.c0 + c.Co], got), \
                        f"{label}: a second launch on the same counters gives other bits"
                    assert ws.counters_zero()
                    assert ws.ok(), f"{label}: a write past the library's split-K workspace size ({ws.nb} bytes)"
            if poisoned:
                assert guards_intact(yb, ya, LIN_SENT[LIN_DT[c.odt]]), \
                    f"{label} block {m}: a y guard was overwritten (columns >= Co, >= ldy, or rows >= B T)"
            res[poisoned, m] = got
        assert same_bits(xb, x0), f"{label}: x or its guards changed"
        if sbuf is not None:
            assert bool(torch.isnan(sbuf[sx.numel():]).all())
    out = []
    for m in range(nblk):
        d = first_diff(res[True, m], res[False, m])
        assert d is None, f"{label} block {m}: poisoned-layout and compact-layout results differ: {d}"
        out.append(res[True, m])
    if staged is not None:
        S = (staged * (448.0 if c.kern == "f8" else 1.0)).to(LIN_DT[c.odt]).to(DEV)
        assert torch.equal(S.float().cpu(), staged * (448.0 if c.kern == "f8" else 1.0)), "the expectation is not exact"
        S = S + 0.0  # (-0 x 448 accumulates to +0)
        for m in range(nblk):
            d = first_diff(out[m], linear_probe_expect(S, c.Co, m))
            assert d is None, f"{label} block {m}: the output is not the staged operand (+0 in columns >= Ci): {d}"
    else:
        for m in range(nblk):
            n = max(0, min(c.Co, c.Ci - m * c.Co))
            assert not bool((out[m][:, :, n:].contiguous().view(torch.int32) != 0).any()), f"{label}: columns >= Ci not +0"
    return torch.cat(out, -1)[:, :, :c.Ci]


@pytest.mark.parametrize("c", [c for c in linear_cases() if c.kern != "glds128"], ids=lin_id)
def test_probe_identity(eng, c):
    """every case of refops.linear_cases but the 128-row tile: assertions 1-6 of the module docstring, exact.  MI355X: all
    110 cases exact (both zeros, the subnormals and +-448 of e4m3 included)."""
    identity(eng, c)


def test_probe_glds_tile128(eng, ncu):
    """gemm_glds on the 128-row tile, reached by shape (STZS_GEMM_TILE is read once per process): the smallest row count
    the launcher's rule (refops.gemm_tile_rows, compared with the launcher's own choice at 256 CUs in
    tests/test_dispatch_trace.py) gives 128-row tiles at Co = 2048, K = 32 -- 64 x 50 rows on 256 CUs -- and 3137 and
    7 x 439 = 3073 rows, whose last tiles hold 65 rows and 1 row.  MI355X (256 CUs): exact."""
    import os
    assert os.environ.get("STZS_GEMM_TILE") is None
    cases = [c for c in linear_cases(ncu) if c.kern == "glds128"]
    if not cases:
        pytest.skip(f"no row count <= 12800 takes the 128-row tile at Co = 2048 on {ncu} CUs")
    for c in cases:
        assert gemm_tile_rows(c.B * c.T, 2048, ncu) == 128
        identity(eng, c)


@pytest.mark.parametrize("kern,Z", [("rows", 2), ("rows16", 0)])
def test_probe_fp32_general_scale(eng, kern, Z):
    """fp32 rows with cscale = 0.37: the staged value is one rounding of the fp32 product, held to bf16 of the fp64
    product by refops.staged_check (ratio <= 1, share of differing bits <= 0.01: the reference alone differs in 0 of
    102 400 elements).  MI355X: ratio 0.9838, share 0 on both forms."""
    import numpy as np
    c = LinCase(kern, 5, 13, 256, 256, Z, "f32", "f32", cscale=0.37)
    S = identity(eng, c).cpu()
    x = lin_make_x(c)[0]
    got = S.to(torch.bfloat16)
    assert torch.equal(got.float(), S), "an fp32 output of a one-hot weight is not a bf16 value"
    s = x.double() * float(np.float32(0.37))
    ratio, share = staged_check(got, s, round_bf16(s), s.abs())
    print(f"{lin_id(c)}: staged max ratio {ratio:.4f}, share of bits differing from bf16(fp64) {share:.3e}")
    assert ratio <= 1, f"staged value off by {ratio:.3f} of the per-element bound"
    assert share <= 0.01


# ------------------------------------------------------------------ B. dense per-element bounds
def guarded_with(h, pads, dt):
    """host values h [B, T, C] inside a poisoned guarded buffer -> its Act"""
    _, a = guarded(tuple(h.shape), pads, LIN_POISON, dt, DEV)
    a.t[:, :, a.c0:a.c0 + h.shape[2]] = h.to(DEV, dt)
    return a


def dense(eng, c, *, act=None, gated=False, acc=False, extra=0, S=None, ops=None, seed=0):
    """one dense launch of a case on the poisoned layout: random bf16-rounded weights / sqrt(K), bias, optionally GELU /
    SiLU, the in-place gated residual (res is y; a gate row per utterance), alpha / beta / acc_in -> the largest ratio
    to the per-element bound (asserted <= 1).  S: the staged operand where it is not x itself."""
    from stzs import _lib as L
    label = f"{lin_id(c)} act {act} gated {gated} acc {acc}"
    dt = LIN_DT[c.odt]
    x, sx, staged = lin_make_x(c, seed) if ops is None else ops
    staged = staged if S is None else S
    g = torch.Generator().manual_seed(7 + c.Ci + c.Co + seed)
    w = torch.randn(c.Co, c.Ci, generator=g) / math.sqrt(c.Ci)
    b = torch.randn(c.Co, generator=g) * 0.1
    if c.kern == "f8":
        from stzs.weights import quantize_f8_cols
        qw, sw = quantize_f8_cols(w)
        cw, wh = pack(c, w, b), qw.float() * sw[:, None]
    else:
        w = bf(w)
        cw, wh = pack(c, w, b), w
    xb, xa = x_layout(c, x, True)
    sbuf, sv = scale_layout(c, sx)
    yb, ya = y_layout(c, True)
    kw, h, gate, ai = {}, None, None, None
    if gated:
        h = torch.randn(c.B, c.T, c.Co, generator=g).to(dt)
        gate = torch.rand(c.B, c.Co, generator=g) + 0.5
        ya.t[:, :, ya.c0:ya.c0 + c.Co] = h.to(DEV)
        gbuf = torch.full((c.B, c.Co + 8), LIN_POISON, device=DEV)
        gbuf[:, :c.Co] = gate.to(DEV)
        kw.update(res=ya, gate=gbuf.data_ptr(), gate_bs=c.Co + 8)
    alpha, beta = (0.75, 1.25) if acc else (1.0, 0.0)
    if acc:
        ai = torch.randn(c.B, c.T, c.Co, generator=g).to(dt)
        kw.update(acc_in=guarded_with(ai, c.ypads, dt), alpha=alpha, beta=beta)
    if act:
        kw["epi_act"] = L.ACT_GELU if act == "gelu" else L.ACT_SILU
    with exact_ws(eng, c, cw) as ws:
        lin_launch(eng, c, cw, xa, ya, x_scale=sv, **kw)
        torch.cuda.synchronize()
        assert ws.ok() and ws.counters_zero(), label
    assert guards_intact(yb, ya, LIN_SENT[dt]), f"{label}: a y guard was overwritten"
    got = ya.t[:, :, ya.c0:ya.c0 + c.Co].cpu()
    K = lin_ci_pad(c) + extra
    z, terms = conv_terms_ref(staged, wh[:, :, None], b, res=h, out_scale=alpha, acc_in=ai, beta=beta, gate=gate)
    if act:
        ratio = act_ratio(got, z, terms, K, act, dt == torch.bfloat16)
    else:
        ratio = dense_ratio(got, z, terms, K, dt == torch.bfloat16)
    print(f"{label}: dense max ratio {ratio:.4f}")
    assert ratio <= 1, f"{label}: {ratio:.3f} of the per-element bound"
    return ratio


@pytest.mark.parametrize("Ci,Z", [(512, 0), (384, 4)])
def test_dense_glds(eng, Ci, Z):
    """gemm_glds bf16 at 129 rows (3 x 43: the 64-row tiles span two utterances), K -> 200 columns: GELU with bf16 out,
    the gated in-place residual with fp32 out (a gate row per utterance), alpha / beta / acc_in with fp32 out; K 384
    in 4 slices (extra = 3).  MI355X largest ratio: GELU bf16 0.88 (K 512), 0.91 (K 384, 4 slices); fp32 out 0.0013 /
    0.0008; the scalar epilogue (Co 22, ldy 24) 0.0010 / 0.0006."""
    ex = max(Z - 1, 0)
    dense(eng, LinCase("glds", 3, 43, Ci, 200, Z, "bf16", "bf16"), act="gelu", extra=ex)
    dense(eng, LinCase("glds", 3, 43, Ci, 200, Z, "bf16", "f32"), gated=True, extra=ex)
    dense(eng, LinCase("glds", 3, 43, Ci, 200, Z, "bf16", "f32"), acc=True, extra=ex)
    dense(eng, LinCase("glds", 3, 43, Ci, 22, Z, "bf16", "f32", (2, 0, 0)), gated=True, extra=ex)  # scalar epilogue


@pytest.mark.parametrize("odt", ["f32", "bf16"])
def test_dense_glds_fp8(eng, odt):
    """gemm_glds fp8 at 129 rows, 320 -> 200: e4m3 rows quantised by the documented quantiser (power-of-two row scales),
    real column scales; the reference is fp64 on the dequantised operands, extra = 2 for acc (sx sw); plain and GELU.
    MI355X largest ratio: fp32 out 0.22 (GELU 0.20), bf16 out 0.96 (GELU 0.90)."""
    c = LinCase("f8", 3, 43, 320, 200, 0, "f8", odt)
    g = torch.Generator().manual_seed(3)
    xr = torch.randn(c.B, c.T, c.Ci, generator=g) * torch.rand(c.B, c.T, 1, generator=g) * 4
    codes, sx = quant_rows_ref(xr)
    S = e4m3_value(codes) * sx[..., None]
    ops = (codes, sx.reshape(-1), S)
    dense(eng, c, extra=2, ops=ops)
    dense(eng, c, act="gelu", extra=2, ops=ops)


# the six CASES rows of tests/test_gpu_rows.py at 129 rows, K <= 512 where the form allows: name, K, N, in, out, act,
# gated residual, acc_in, cscale, Z on gemm_rows, Z on rows16
SMALL_M = [("qkv", 512, 1536, "bf16", "bf16", None, False, False, 1.0, 2, 0),
           ("ff1", 512, 2048, "bf16", "bf16", "gelu", False, False, 1.0, 0, 0),
           ("o", 512, 512, "bf16", "f32", None, True, False, 1.0, 4, 4),
           ("ff2", 512, 512, "bf16", "f32", None, True, False, 1.0, 2, 0),
           ("out", 512, 256, "bf16", "f32", None, False, True, 1.0, 0, 4),
           ("in", 256, 512, "f32", "f32", None, False, False, 0.37, 2, 2)]


@pytest.mark.parametrize("kern", ["rows", "rows16"])
@pytest.mark.parametrize("case", SMALL_M, ids=[r[0] for r in SMALL_M])
def test_dense_small_m(eng, kern, case):
    """gemm_rows and rows16 on the denoiser's six linear forms at 129 rows (extra = 3 wave partials on gemm_rows, + Z - 1
    slices); the fp32-input form against fp64 on the staged operand its own probe returned.  MI355X largest ratio: bf16
    out 0.90 (qkv), 0.91 (GELU ff1) on both kernels; fp32 out 0.0006 .. 0.0016."""
    name, K, N, idt, odt, act, gated, acc, cs, zr, z16 = case
    Z = zr if kern == "rows" else z16
    c = LinCase(kern, 3, 43, K, N, Z, idt, odt, cscale=cs)
    S = None
    if idt == "f32":
        S = identity(eng, LinCase(kern, 3, 43, K, K, Z, idt, "f32", cscale=cs)).cpu()
    dense(eng, c, act=act, gated=gated, acc=acc, extra=(3 if kern == "rows" else 0) + max(Z - 1, 0), S=S)


# ------------------------------------------------------------------ C. ln_rows against fp64
LN_ROWS = {1: (1, 1), 15: (3, 5), 17: (17, 1), 129: (3, 43)}


def ln_setup(eng, K, idt, R, form, seed=0):
    """rows h [R, K] inside a flat buffer with ldx = K + 8 (poison behind every row and behind the last), the
    modulation of `form` ("adaln": a (G, Bt) row per utterance, gdiv = T -- groups change inside a 16-row block;
    "affine": one vector, gs = bs = 0) -> (stzs_rowln_args, the Act the engine routes on, fp64 reference, terms, keep)"""
    from stzs.engine import Act
    B, T = LN_ROWS[R]
    dt = LIN_DT[idt]
    g = torch.Generator().manual_seed(seed + K + R)
    h = (torch.randn(R, K, generator=g) * 2 + 0.3).to(dt)
    hb = torch.full((B, T + 1, K + 8), LIN_POISON, dtype=dt, device=DEV)
    hb.view(-1, K + 8)[:R, :K] = h.to(DEV)
    hv = Act(hb.view(1, -1, K + 8)[:, :R], 0, K)
    ng = B if form == "adaln" else 1
    G = torch.randn(ng, K, generator=g) * 0.2
    Bt = torch.randn(ng, K, generator=g) * 0.1
    gs = K + 8 if form == "adaln" else 0
    Gd = torch.full((ng, K + 8), LIN_POISON, device=DEV)
    Bd = torch.full((ng, K + 8), LIN_POISON, device=DEV)
    Gd[:, :K], Bd[:, :K] = G.to(DEV), Bt.to(DEV)
    gadd = 1.0 if form == "adaln" else 0.0
    xln = Act(torch.zeros(B, T, K, dtype=torch.bfloat16, device=DEV))  # (the unfused form's output: never written)
    ln = eng._ln_args(hv, xln, G=Gd.data_ptr(), gs=gs, Bt=Bd.data_ptr(), bs=gs, gdiv=T if form == "adaln" else 1, gadd=gadd)
    grp = torch.arange(R) // T if form == "adaln" else torch.zeros(R, dtype=torch.long)
    ref, terms = layernorm_ref64(h.float(), G, Bt, grp, gadd)
    return ln, xln, ref, terms, (hb, Gd, Bd, B, T)


def ln_launch(eng, cw, ln, xln, ya, **kw):
    """the fused launch through the engine: one launch, entry point stzs_ln_linear with the LayerNorm fused"""
    rec, entry = [], eng._conv_entry
    eng._conv_entry = lambda *a, **k: rec.append(entry(*a, **k)) or rec[-1]
    n0 = eng.launches
    try:
        eng.conv(cw, xln, ya, rows=1, pre_ln=ln, what="lnrows", **kw)
    finally:
        eng._conv_entry = entry
    torch.cuda.synchronize()
    assert rec[0][0] is eng.lib.stzs_ln_linear and rec[0][2] and eng.launches == n0 + 1, "not the fused ln_rows launch"


def ln_image(eng, K, idt, R, form):
    """-> (the operand image [R, K] bf16 (host), the setup): identity weight, fp32 out, guarded y"""
    ln, xln, ref, terms, keep = ln_setup(eng, K, idt, R, form)
    B, T = keep[3:]
    c = LinCase("ln", B, T, K, K, 0, idt, "f32")
    cw = pack(c, torch.eye(K), None, key=("eye", K))
    yb, ya = y_layout(c, True)
    ln_launch(eng, cw, ln, xln, ya)
    assert guards_intact(yb, ya, LIN_SENT[torch.float32]), "ln_rows: a y guard was overwritten"
    y = ya.t[:, :, ya.c0:ya.c0 + K].reshape(R, K).cpu()
    img = y.to(torch.bfloat16)
    assert torch.equal(img.float(), y), "the image read through an identity weight is not a bf16 value"
    return img, (ln, xln, ref, terms, keep)


@pytest.mark.parametrize("form", ["adaln", "affine"])
@pytest.mark.parametrize("idt", ["f32", "bf16"])
@pytest.mark.parametrize("K", [128, 256, 512])
def test_ln_rows_image_vs_fp64(eng, K, idt, form):
    """the fused operand image against an fp64 LayerNorm of the stored rows (not against another kernel), R = 1, 15, 17,
    129, ldx = K + 8 with poison behind the row: within one bf16 ulp of the rounded reference, or within 2^-8 |ref| +
    64 2^-24 terms (test_row_layernorm_edges' rule).  MI355X: at most 1 bf16 ulp from the rounded reference in all 48
    (K, dtype, R, form) cases, no element past one."""
    for R in LN_ROWS:
        img, (_, _, ref, terms, _) = ln_image(eng, K, idt, R, form)
        ok, umax, past = layernorm_image_ok(img, ref, terms)
        print(f"ln_rows K{K} {idt} R{R} {form}: max {umax} bf16 ulp from the rounded reference, {past} past one")
        assert ok, f"ln_rows K{K} {idt} R{R} {form}: the operand image is not the fp64 LayerNorm ({umax} ulp)"


@pytest.mark.parametrize("K", [128, 256, 512])
def test_ln_rows_dense(eng, K):
    """dense launches (K -> 200: GELU bf16 out, SiLU bf16 out, alpha / beta / acc_in fp32 out, plain fp32 out) at 129
    adaLN rows against fp64 on the image just read (the two-stage scheme): dense_ratio / act_ratio <= 1.  MI355X largest
    ratio: GELU / SiLU bf16 0.96 (K 128), 0.95 (K 256), 0.86 (K 512); fp32 out 0.0064, 0.0024, 0.0015."""
    from stzs import _lib as L
    img, (ln, xln, _, _, keep) = ln_image(eng, K, "f32", 129, "adaln")
    B, T = keep[3:]
    S = img.float().view(B, T, K)
    g = torch.Generator().manual_seed(K)
    w = bf(torch.randn(200, K, generator=g) / math.sqrt(K))
    b = torch.randn(200, generator=g) * 0.1
    for act, odt, acc in (("gelu", "bf16", False), ("silu", "bf16", False), (None, "f32", True), (None, "f32", False)):
        c = LinCase("ln", B, T, K, 200, 0, "f32", odt)
        dt = LIN_DT[odt]
        cw = pack(c, w, b)
        yb, ya = y_layout(c, True)
        kw, ai = {}, None
        if acc:
            ai = torch.randn(B, T, 200, generator=g)
            kw.update(acc_in=guarded_with(ai, c.ypads, dt), alpha=0.75, beta=1.25)
        if act:
            kw["epi_act"] = L.ACT_GELU if act == "gelu" else L.ACT_SILU
        ln_launch(eng, cw, ln, xln, ya, **kw)
        assert guards_intact(yb, ya, LIN_SENT[dt])
        got = ya.t[:, :, ya.c0:ya.c0 + 200].cpu()
        z, terms = conv_terms_ref(S, w[:, :, None], b, out_scale=0.75 if acc else 1.0, acc_in=ai, beta=1.25 if acc else 0.0)
        ratio = act_ratio(got, z, terms, K, act, True) if act else dense_ratio(got, z, terms, K, odt == "bf16")
        print(f"ln_rows dense K{K} act {act} {odt} acc {acc}: max ratio {ratio:.4f}")
        assert ratio <= 1
