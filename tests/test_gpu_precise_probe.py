"""Precise (split-operand) register-direct convs: exact operand probes and exact-sum dense checks (csrc/mrfx.hip mrfx_conv
-- Snake, LeakyReLU / identity k3 and the narrow conv_post form -- and mrfx_lin).

The kernels stage pro(x) as the pair hi = bf16(z), lo = bf16(z - hi) and form w z as wl zh + wh zl + wh zh with fp32
accumulation.  hi + lo is exact in fp32, so a one-hot weight 1.0 (refops.delta_weights), bias 0, no residual and alpha 1
make the fp32 output the staged PAIR, bit for bit (every other product is 0 * finite): one launch per (tap, channel
block) reads the staged tensor out through every (tile, staged row, tap) pairing, chunk, wave and the weight-packing
permutation.  Each probe launch runs on poisoned operands (finite 2^100 around x at channel offset 8, 8 more columns, 3
more rows per utterance, non-compact stat_bs / gb_bs / gb_beta_off, a NaN-sentinel guarded output) and on compact
zero-padded ones; both must agree in bits, every guard must be intact and x untouched.  One-hot weights 1 + 2^-9 (wh =
1, wl = 2^-9) then pin the lo weight fragment, and exact-sum operands (refops.exact_sum_case: values a + b 2^-10) make
every product and partial sum exactly representable, so a dense launch with the full epilogue must equal the fp64 sum
of the three products bit for bit: a dropped, doubled or mis-paired product at any K-step, tap, chunk or wave changes
bits.  The Snake prologue is inexact, so the Snake instantiations (every k7 / k11 form, the 64-row tiles, the single-
chunk template) are held to the identity probes and to the per-element bound refops.x3_dense_ratio on random operands;
the LeakyReLU / identity k3 template, the narrow form and mrfx_lin (no activation) are held to bit equality.

Which tile height each case runs is asserted without a device by tests/test_dispatch_trace.py (k7 d5 runs 128-row
tiles: 158 staged rows <= 16 sb_rows(7, 128) = 160).  Measured figures stand in each test's docstring.

Measured on MI355X: every exact read-out, lo-plane identity and exact-sum launch is bit-exact (the MFMA keeps exactly
representable multi-term sums exact: the derived fallback bound was not needed).

Mutations of csrc/mrfx.hip (scratch builds, each run once on MI355X; "old" = the 20 mrfx kernel tests of
tests/test_gpu_precise.py):
  bq * a.stat_bs -> bq * a.Ci (AdaIN rows)        -> 53 tests here ("conv-2x5-128to128-k3d1-snake-t128: tap 0 block 0:
                                                     poisoned-layout and compact-layout results differ"); old: all GREEN
  mrfx_lin: qq * a.bsx -> qq * a.T_in * a.ldx     -> 26 tests here ("lin-3x50-128to136-k1d1-none-t128: tap 0 block 0:
                                                     poisoned-layout and compact-layout results differ"); old: all GREEN
  wl fragment of the other row tile, w[2 + (1-j)] -> 20 tests here, no identity probe (wl = 0 there): test_lo_plane_identity
                                                     ("not x (1 + 2^-9): 68058 elements differ"), test_exact_sum ("not the
                                                     exact three-product sum: 16432 elements differ"), test_dense; old: 13 red
  lo store skipped for staged row rows_in - 1     -> 50 tests here ("tap 2: zero padding not +0 at utterance 0 output row
                                                     127"); old: 13 red
None faulted."""
import math

import pytest
import torch

import refops as R
from refops import (adain_consts, conv_terms_ref, delta_weights, delta_weights_T, fill_bits, first_diff, guards_intact,
                    pro_ref64, probe_readout, probe_readout_T, same_bits)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = R.precise_probe_cases()


@pytest.fixture(scope="module")
def eng(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    yield StyleTTSZS(tiny, tiny_params, device=gpu_device)
    _PROBED.clear()
    R.PX_PACKED.clear()


def _sent(shape):
    return fill_bits(shape, torch.float32, R.PX_SENT, DEV)


_PROBED = {}


def probe(eng, c, seed=0, scale=1.0, x=None):
    """the staged pair of a case read through every tap and channel block with one-hot weights of value `scale`, on the
    poisoned layout; every launch repeated on the compact layout.  Asserts: return code 0, same bits on both layouts,
    padding rows and channels >= Ci +0, read-outs of one staged row through different taps agree, y guards intact
    (the narrow form: columns [Co, ceil8(Co)) too), x untouched -> (read-out [B, T, Ci] on the host, operands)"""
    k0 = (c, seed, scale, x is None)
    if k0 in _PROBED:
        return _PROBED[k0]
    o = R.px_make_ops(c, seed)
    if x is not None:
        o["x"] = x
    dp, dc = R.px_layout(c, o, True, DEV), R.px_layout(c, o, False, DEV)
    x_before = dp["xb"].clone()
    label, problems = R.px_id(c), []

    def run(j0, m):
        w = delta_weights_T(c.Ci, c.Co, c.k, j0, m) if c.ups else delta_weights(c.Co, c.Ci, c.k, j0, m)
        cw = R.px_pack(c, w * scale, None, (c.kern, c.Co, c.Ci, c.k, c.ups, j0, m, scale), DEV)
        (yb, ya), (ycb, yc) = R.px_y(c, True, DEV), R.px_y(c, False, DEV)
        R.px_launch(eng, R.px_args(eng, c, cw, dp, ya))
        R.px_launch(eng, R.px_args(eng, c, cw, dc, yc))
        torch.cuda.synchronize()
        if not guards_intact(yb, ya, R.PX_SENT):
            problems.append(f"tap {j0} block {m}: a y guard was overwritten")
        if bool((ycb[:, :, c.Co:] != 0).any()):
            problems.append(f"tap {j0} block {m}: compact output columns >= Co written")
        got = ya.t[:, :, ya.c0:ya.c0 + c.Co].clone()
        if not same_bits(got, yc.t[:, :, :c.Co]):
            problems.append(f"tap {j0} block {m}: poisoned-layout and compact-layout results differ")
        return got

    if c.ups:
        S, pr = probe_readout_T(run, T=c.T, Ci=c.Ci, Co=c.Co, ups=c.ups, ups_pad=c.ups // 2, refl=c.refl)
    else:
        S, pr = probe_readout(run, T=c.T, Ci=c.Ci, Co=c.Co, k=c.k, dil=c.dil, pad=R.px_pad(c), stride=c.stride, tile=c.tile)
    assert not (problems + pr), label + ": " + "; ".join((problems + pr)[:6])
    assert same_bits(dp["xb"], x_before), label + ": x was written"
    _PROBED[k0] = (S.cpu(), o)
    return _PROBED[k0]


def check_staged(S, c, o):
    """the read-out against the prologue: bit equality with refops.x3_identity_expect for the exact prologues, else
    refops.x3_staged_ratio <= 1 against the fp64 prologue -> the ratio (0.0 for an exact prologue)"""
    adain, act, slope, exact = R.PX_PRO[c.pro]
    label = R.px_id(c)
    if exact:
        sc, sh = R.px_consts(o)
        d = first_diff(S, R.x3_identity_expect(o["x"] * c.cscale, sc, sh, act, slope))
        assert d is None, f"{label}: the read-out differs from hi + lo of the exact prologue: {d}"
        return 0.0
    sc = sh = None
    if adain:
        sc, sh = adain_consts(*(o[n] for n in ("mean", "rstd", "gamma", "beta")))
    s, _, mag = pro_ref64(o["x"], sc, sh, act, slope, o["alpha"])
    ratio = R.x3_staged_ratio(S, s, mag)
    print(f"{label}: staged max ratio {ratio:.4f}")
    assert ratio <= 1, f"{label}: staged pair off by {ratio:.3f} of the per-element bound"
    return ratio


# ------------------------------------------------------------------ a. identity probes
@pytest.mark.parametrize("c", [c for c in CASES if c.kern in ("conv", "narrow")], ids=R.px_id)
def test_probe_mrfx_conv(eng, c):
    """mrfx_conv: single- and multi-chunk Snake forms on 128-row and 64-row tiles, the LeakyReLU / identity k3 forms
    (130 -> 64: ci_pad 256, one valid vector with 2 valid channels in the second chunk) and the narrow conv_post form
    (masked stores past Co = 22).  Exact prologues: the read-out IS hi + lo of the exact fp32 prologue value, bit for bit.
    MI355X, inexact prologues (|S - s| over 2^-17 |s| + 2^-20 magnitude): AdaIN + Snake (v_sin_f32 on revolutions) <=
    0.8825, AdaIN + LeakyReLU(0.2) 0.8803, LeakyReLU(0.01) 0.8866 -- the split's own truncation."""
    S, o = probe(eng, c)
    check_staged(S, c, o)


@pytest.mark.parametrize("c", [c for c in CASES if c.kern == "lin"], ids=R.px_id)
def test_probe_mrfx_lin(eng, c):
    """mrfx_lin: K 128 .. 640 (the next-chunk register prefetch) and 200 (whole vectors past Ci), rows straddling
    utterances on a non-compact bsx, a partial last tile, T_in = 1 (B = 64), Co 8 / 136 / 600, cscale 1 and 0.5: the
    read-out is hi + lo of x cscale, bit for bit."""
    S, o = probe(eng, c)
    check_staged(S, c, o)


@pytest.mark.parametrize("c", [c for c in CASES if c.kern.startswith("x3")], ids=R.px_id)
def test_probe_conv_x3(eng, c):
    """conv_x3, fp32 in and out (the only dtype pair the precise engines launch): k5 with every prologue instantiation
    (Snake by libm sinf; 90 channels: 2 valid in the last vector), the FLAT k1 form (Ci 48, rows straddling utterances,
    T_in = 1), the stride-6 k12 conv at T = 800 (774 staged rows: the tight 64-byte row pitch) and the polyphase
    ConvTransposes ups 6 / 10 with and without the reflection row (refops.probe_readout_T: every output row is one staged
    row or +0, nothing written at t >= T_final + refl).  MI355X staged ratios: Snake 0.8656 (stride-6: 0.8605), LeakyReLU(0.1)
    0.8866 (ConvTranspose: 0.8866)."""
    S, o = probe(eng, c)
    check_staged(S, c, o)


# ------------------------------------------------------------------ b. lo-plane identity
LO = 1.0 + 2.0 ** -9  # wh = 1, wl = 2^-9


@pytest.mark.parametrize("c", [R.PxCase("conv", 2, 129, 264, 128, 3, 1, "none", 128), R.PxCase("lin", 2, 129, 256, 136),
                               R.PxCase("x3", 2, 129, 90, 80, 5, 1, "none")], ids=R.px_id)
def test_lo_plane_identity(eng, c):
    """one-hot weights 1 + 2^-9 on bf16-representable x (zl = 0) with no prologue: the output must be x (1 + 2^-9)
    exactly (17 significant bits) through every tap and block -- the lo weight fragment (p[512], p[576]; conv_x3: the
    second stream of kstep_stream_x3) sits at its tap, K-step, wave and lane."""
    g = torch.Generator().manual_seed(3)
    x = R.bf(torch.randn(c.B, c.T, c.Ci, generator=g))
    S, _ = probe(eng, c, scale=LO, x=x)
    d = first_diff(S, (x.double() * LO).float())
    assert d is None, f"{R.px_id(c)}: not x (1 + 2^-9): {d}"


def test_lo_plane_identity_snake(eng):
    """the k7 d3 single-chunk form exists with the Snake prologue only, whose staged lo is not 0: the output is S + 2^-9
    zh, up to 25 significant bits, so it is held to one fp32 rounding of that value (2^-24 of it), with zh = bf16(S) or,
    where S sits exactly at a bf16 tie, its other neighbour (refops fact 2).  A lo weight fragment of another tap, K-step
    or lane reads another staged value: 2^-9 of a different number."""
    c = R.PxCase("conv", 2, 129, 128, 128, 7, 3, "snake", 128)
    S, _ = probe(eng, c)
    Y, _ = probe(eng, c, scale=LO)
    hi, lo, _ = R.split_ref(S)
    Sd, Yd = S.double(), Y.double()
    want = Sd + 2.0 ** -9 * hi.double()
    e = (Yd - want).abs()
    ok = e <= 2.0 ** -24 * want.abs()
    hb = hi.to(torch.bfloat16).view(torch.int16).to(torch.int32)  # the bf16 neighbour of zh on lo's side
    alt = (hb + torch.where(torch.sign(lo) == torch.sign(hi), 1, -1)).to(torch.int16).view(torch.bfloat16).double()
    tie = (Sd - hi.double()).abs() == (alt - Sd).abs()
    want2 = Sd + 2.0 ** -9 * alt
    ok |= tie & ((Yd - want2).abs() <= 2.0 ** -24 * want2.abs())
    assert bool(ok.all()), (f"{int((~ok).sum())} elements are not S + 2^-9 zh; first at {tuple(int(v) for v in (~ok).nonzero()[0])}, "
                            f"off by {float((e / Sd.abs().clamp_min(1e-30))[~ok].max()):.3e} of |S|")


# ------------------------------------------------------------------ c. exact-sum dense launches
def _dense_launch(eng, c, w, b, o, *, res=None, res_tdiv=1, acc=None, alpha=1.0, beta=0.0, gate=None, stat=False):
    """one dense launch on the poisoned layout with res / acc_in / gate in guarded buffers of their own and, with
    stat, a sentinel-filled statistics slab with stat_ld > Co and one chunk row more than the conv has -> (y on the
    host, the slab's partials [B, nch, Co, 2] | None).  Asserts the return code, the y guards, x / res / acc_in
    untouched and the slab outside [B, nch, Co] untouched."""
    label = R.px_id(c)
    a, k = R.px_dense_args(eng, c, w, b, o, DEV, res=res, res_tdiv=res_tdiv, acc=acc, alpha=alpha, beta=beta, gate=gate,
                           stat=stat)
    d, ro, yb, ya, slab, nch = k["d"], k["ro"], k["yb"], k["ya"], k["slab"], k["nch"]
    before = [t.clone() for t in (d["xb"], ro[0][0], ro[1][0]) if t is not None]
    R.px_launch(eng, a)
    torch.cuda.synchronize()
    assert guards_intact(yb, ya, R.PX_SENT), label + ": a y guard was overwritten"
    after = [t for t in (d["xb"], ro[0][0], ro[1][0]) if t is not None]
    assert all(same_bits(p, q) for p, q in zip(before, after)), label + ": a read-only operand was written"
    part = None
    if stat:
        chk = slab.clone()
        chk[:c.B * nch, :c.Co] = _sent((c.B * nch, c.Co, 2))
        assert same_bits(chk, _sent(chk.shape)), label + ": statistics written outside [B, chunks of T_out, Co]"
        part = slab[:c.B * nch, :c.Co].view(c.B, nch, c.Co, 2).cpu()
    return ya.t[:, :, ya.c0:ya.c0 + c.Co].cpu(), part


def _check_stats(part, got, T, label):
    """the fused statistics partials (sum v, sum v^2 per 64-row chunk, read straight from stat_part) against fp64 sums of
    the stored y: within 64 2^-24 sum |v| and 64 2^-24 sum v^2"""
    y = got.double()
    for i, v in enumerate((y, y * y)):
        for ch in range((T + 63) // 64):
            sl = slice(ch * 64, (ch + 1) * 64)
            err = (part[:, ch, :, i].double() - v[:, sl].sum(1)).abs()
            bound = 64 * 2.0 ** -24 * v[:, sl].abs().sum(1)
            assert bool((err <= bound).all()), (f"{label}: statistics partial {i} of chunk {ch} off by "
                                                f"{float((err / bound.clamp_min(1e-300)).max()):.3f} of its bound")


@pytest.mark.parametrize("case", R.precise_exact_cases(), ids=R.px_exact_id)
def test_exact_sum(eng, case):
    """exact-sum operands (values a + b 2^-10), dense weights, integer bias and the full epilogue with dyadic constants on
    the poisoned layout: bit equality with refops.x3_terms_ref (the fp64 sum of wl zh + wh zl + wh zh on the real split),
    zeros compared without their sign.  Instantiations held to bit equality: mrfx_conv<LEAKY | NONE, residual, false, 3,
    128, 0, true> (130 -> 64 with and without residual, res_tdiv = 2 at odd T; 1090 -> 256: 9 chunks, |a|, |c| <= 1;
    LeakyReLU with the exact slope 2), the narrow conv_post form, and mrfx_lin<NONE, gate, residual, accumulate> in all 8
    combinations plus the broadcast residual (bsr = 0) and K 640; conv_x3 at k5 (full epilogue, LeakyReLU), FLAT with gate +
    residual, stride 6 on the tight row pitch and the polyphase ConvTranspose with its reflection row.  The Snake instantiations (every k7 / k11 form, the
    64-row tiles, NCH = 1) have no exact prologue: they are held to test_dense (section d) and the identity probes.
    Fused statistics: 64 2^-24 sum |v| / sum v^2 per 64-row chunk; nothing written past the chunks of T_out."""
    c, seed, e = case
    ops, pro = R.px_exact_operands(c, seed, e)
    o = dict(x=ops["x"], mean=None, alpha=None)
    w = ops["w"].transpose(0, 1).contiguous() if c.ups else ops["w"]  # (the ConvTranspose1d layout [Ci, Co, k])
    got, part = _dense_launch(eng, c, w, ops["b"], o, res=ops["res"], res_tdiv=e["res_tdiv"], acc=ops["acc"],
                              alpha=e["alpha"], beta=e["beta"], gate=ops["gate"], stat=e["stat"])
    d = first_diff(got + 0.0, R.px_exact_ref(c, ops, pro, e) + 0.0)
    assert d is None, f"{R.px_exact_id(case)}: not the exact three-product sum: {d}"
    if e["stat"]:
        _check_stats(part, got, R.px_T_out(c), R.px_exact_id(case))


# ------------------------------------------------------------------ d. random dense launches, the real prologues
@pytest.mark.parametrize("case", R.precise_dense_cases(), ids=R.px_dense_id)
def test_dense(eng, case):
    """random fp32 weights on the probed operands of the real prologues (general AdaIN + Snake on every Snake tile form,
    AdaIN + LeakyReLU(0.2), mrfx_lin with gate + residual + accumulate) against ref_full = sum w S in fp64 on the
    read-out S: per element within (2^-16 + 2^-17 + 2 (3K + 4) 2^-24) terms (refops.x3_dense_ratio <= 1); fused statistics
    by the rule of test_exact_sum.  MI355X largest ratio: mrfx_conv Snake 0.0035 (128-row single chunk 0.0033, 64-row k11 d3
    0.0014, 256 -> 256 0.0035, 384 -> 176 0.0004), AdaIN + LeakyReLU(0.2) 0.0088, mrfx_lin 0.0035; conv_x3 k5 Snake 0.0065,
    stride-6 0.0142, ConvTranspose 0.0219."""
    c, e = case
    S, o = probe(eng, c)
    d = R.px_dense_operands(c, e)
    got, part = _dense_launch(eng, c, d["w"], d["b"], o, res=d["res"], res_tdiv=e["res_tdiv"], acc=d["acc"],
                              alpha=e["alpha"], beta=e["beta"], gate=d["gate"], stat=e["stat"])
    ref, terms, K = R.px_dense_ref(c, S, d, e)
    ratio = R.x3_dense_ratio(got, ref, terms, K)
    print(f"{R.px_dense_id(case)}: dense max ratio {ratio:.4f}")
    assert ratio <= 1, f"{R.px_dense_id(case)}: {ratio:.3f} of the per-element bound"
    if e["stat"]:
        _check_stats(part, got, R.px_T_out(c), R.px_dense_id(case))


@pytest.mark.parametrize("act", ["gelu", "silu"])
def test_dense_lin_act(eng, act):
    """mrfx_lin with the GELU / SiLU epilogue (libm erff / expf), 3 x 50 rows, K 256 -> 136: refops.act_ratio with K -> 3K
    on the pre-activation sum w S.  MI355X: GELU 0.0138, SiLU 0.0126."""
    from stzs import _lib as L
    c = R.PxCase("lin", 3, 50, 256, 136)
    S, o = probe(eng, c)
    g = torch.Generator().manual_seed(21)
    w = torch.randn(c.Co, c.Ci, 1, generator=g) / math.sqrt(c.Ci)
    b = torch.randn(c.Co, generator=g) * 0.1
    a, k = R.px_dense_args(eng, c, w, b, o, DEV, epi_act=L.ACT_GELU if act == "gelu" else L.ACT_SILU)
    yb, ya = k["yb"], k["ya"]
    R.px_launch(eng, a)
    torch.cuda.synchronize()
    assert guards_intact(yb, ya, R.PX_SENT)
    z, terms = conv_terms_ref(S, w, b)
    ratio = R.act_ratio(ya.t[:, :, ya.c0:ya.c0 + c.Co].cpu(), z, terms, 3 * c.Ci, act, False)
    print(f"mrfx_lin {act}: max ratio {ratio:.4f}")
    assert ratio <= 1
