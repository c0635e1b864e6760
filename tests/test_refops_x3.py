"""The split-operand references of tests/test_gpu_precise_probe.py, proven on the CPU: the three facts the exact checks
rest on, a value-level fp32 emulation of the kernel arithmetic (refops.x3_emulate) that meets bit equality on every
exact-sum case of the GPU table in three accumulation orders, and value-only mistakes planted in the emulation that
each turn the corresponding check red."""
import pytest
import torch

import refops as R
from refops import first_diff, pro_ref64, split_ref


def _edge_values():
    """powers of two, values just under a binade, tie-valued lo, zeros, negative zeros"""
    p2 = 2.0 ** torch.arange(-20, 21).float()
    under = torch.nextafter(p2, torch.zeros_like(p2))
    hi = torch.tensor([1.0, 1.5, 3.0, 100.0, 0.0078125])
    tie = torch.cat([hi + 2.0 ** -8 * hi.abs().log2().floor().exp2(), hi * (1 + 2.0 ** -8), hi * (1 + 2.0 ** -8 + 2.0 ** -16)])
    v = torch.cat([p2, under, tie, torch.tensor([0.0, -0.0])])
    return torch.cat([v, -v])


def test_fact1_sum_exact_and_close():
    """hi + lo is exactly representable in fp32 and |z - (hi + lo)| <= 2^-17 |z|; with a one-hot weight 1.0 the three
    products 0 + wl zh + wh zl + wh zh in fp32 are hi + lo bit for bit"""
    g = torch.Generator().manual_seed(0)
    z = torch.cat([torch.randn(2_000_000, generator=g) * torch.exp2(torch.randint(-30, 30, (2_000_000,), generator=g).float()),
                   _edge_values()])
    hi, lo, S = split_ref(z)
    assert bool((hi.double() + lo.double() == S.double()).all())
    err = (z.double() - S.double()).abs()
    assert bool((err <= 2.0 ** -17 * z.abs().double()).all()), float((err / z.abs().double().clamp_min(1e-300)).max())
    wh, wl, _ = split_ref(torch.ones(()))
    assert float(wh) == 1.0 and float(wl) == 0.0
    acc = torch.zeros_like(z) + wl * hi
    acc = acc + wh * lo
    acc = acc + wh * hi
    assert first_diff(acc + 0.0, S + 0.0) is None


def test_fact2_resplit_differs_only_at_ties():
    """re-splitting S = hi + lo returns the same pair except where S sits at a bf16 tie (about 1e-3 of random values):
    references must split the prologue value themselves"""
    g = torch.Generator().manual_seed(1)
    z = torch.randn(2_000_000, generator=g)
    hi, lo, S = split_ref(z)
    hi2, lo2, S2 = split_ref(S)
    assert bool((S2 == S).all())
    diff = hi2 != hi
    share = diff.double().mean().item()
    assert 0 < share < 5e-3, share
    half = R.half_ulp_bf16(hi.double())
    # (a changed hi: lo rounded up to half a spacing of hi, or hi a power of two approached from below)
    assert bool(((lo.double().abs() >= half / 2) | ~diff).all())


def test_fact3_exact_sum_operands_split_as_stated():
    """values a + b 2^-10: hi = a and lo = b 2^-10 wherever a != 0; the case's condition holds for the GPU table"""
    for K, B, T, Ci, Co, k in ((1408, 1, 4, 128, 8, 11), (3270, 1, 4, 1090, 8, 3)):
        e = R.exact_sum_case(K, 5, B=B, T=T, Ci=Ci, Co=Co, k=k)
        for v in (e["x"], e["w"]):
            hi, lo, S = split_ref(v)
            a = torch.round(v)
            nz = a != 0
            assert bool((hi[nz] == a[nz]).all()) and bool((lo[nz] == (v - a)[nz]).all()) and bool((S == v).all())
            assert float(v.abs().max()) <= (2 if K <= 1408 else 1) + 3 * 2.0 ** -10
    with pytest.raises(AssertionError):
        R.exact_sum_case(9000, 5, B=1, T=4, Ci=3000, Co=8, k=3, alpha=0.5, res=True)  # (past 2^13)


def test_identity_expect_edges():
    """x3_identity_expect on the exact prologues: S of x sc (power of two) through LeakyReLU 1/8; -0 reads out as +0"""
    x = _edge_values().view(1, -1, 1).repeat(2, 1, 3)
    sc = torch.tensor([[1.0, 2.0, 0.25], [4.0, 0.5, 1.0]])
    E = R.x3_identity_expect(x, sc, torch.zeros(2, 3), "leaky", 0.125)
    v = x.double() * sc.double()[:, None, :]
    v = torch.where(v >= 0, v, v / 8)
    assert first_diff(E, split_ref(v.float())[2]) is None
    assert bool((R.x3_identity_expect(torch.full((1, 1, 1), -0.0)).view(torch.int32) == 0).all())


def _emulate_case(c, ops, pro, e, order, mutate=None):
    rr = ops["res"].expand(c.B, -1, -1) if ops["res"] is not None else None
    return R.x3_emulate(ops["x"], ops["w"], ops["b"], act=pro["act"], slope=pro["slope"], pad=R.px_pad(c),
                        dil=c.dil, stride=c.stride, ups=c.ups, ups_pad=c.ups // 2, refl=c.refl, res=rr, res_tdiv=e["res_tdiv"], out_scale=e["alpha"], acc_in=ops["acc"], beta=e["beta"],
                        gate=ops["gate"], order=order, mutate=mutate)[0]


@pytest.mark.parametrize("case", R.precise_exact_cases(), ids=R.px_exact_id)
def test_emulation_exact_in_three_orders(case):
    """the emulation (three bf16 products per term, torch.float32 accumulation) equals x3_terms_ref bit for bit on every
    exact-sum case of the GPU table: tap-major sequential, reversed, and blocked by 32-wide K-step.  (The sequential
    orders run on the first utterance and 24 output channels of the wide cases: the property is per element.)"""
    c, seed, e = case
    ops, pro = R.px_exact_operands(c, seed, e)
    ref = R.px_exact_ref(c, ops, pro, e)
    assert first_diff(_emulate_case(c, ops, pro, e, "blk32") + 0.0, ref + 0.0) is None
    if c.Ci * c.k > 640:  # (a slice of the problem: K sequential steps over every output element cost seconds)
        n = 24 if c.Co > 24 else c.Co
        cut = lambda t, d: t if t is None else t.narrow(d, 0, n)
        sub = dict(ops, x=ops["x"][:1], w=ops["w"][:n], b=ops["b"][:n], res=None if ops["res"] is None else cut(ops["res"][:1], 2),
                   acc=None if ops["acc"] is None else cut(ops["acc"][:1], 2), gate=None if ops["gate"] is None else cut(ops["gate"][:1], 1))
        c, ops, ref = c._replace(B=1, Co=n), sub, ref[:1, :, :n]
    for order in ("seq", "rev"):
        assert first_diff(_emulate_case(c, ops, pro, e, order) + 0.0, ref + 0.0) is None, order


def _first_msg(fn):
    with pytest.raises(AssertionError) as ei:
        fn()
    return str(ei.value).split("\n")[0]


def _exact_check(c, seed, e, mutate, order="blk32"):
    ops, pro = R.px_exact_operands(c, seed, e)
    d = first_diff(_emulate_case(c, ops, pro, e, order, mutate) + 0.0, R.px_exact_ref(c, ops, pro, e) + 0.0)
    assert d is None, f"not the exact three-product sum: {d}"


def test_mutations_turn_the_exact_sum_check_red():
    """value-only mistakes in the emulation against the exact-sum check (130 -> 64 k3, res_tdiv 2, alpha 0.5), with the
    first message of each:
      wl zh dropped in one K-step       -> "not the exact three-product sum: 15992 elements differ; first at (utterance,
                                            row, column) (0, 1, 0): got 16.49267578125, expected 16.48388671875"
      lo plane of tap 0 at tap 1's rows -> "... 16361 elements differ; first at ... (0, 0, 0): got 3.99560546875, expected
                                            3.98095703125"
      staged lo row 3 taken from row 4  -> "... 381 elements differ; first at ... (0, 2, 0): got -2.9990234375, expected
                                            -2.9716796875"
      wl zl added                       -> "... 16124 elements differ; first at ... (0, 0, 0): got 3.980935573577881,
                                            expected 3.98095703125"
      res_tdiv ignored                  -> "... 14459 elements differ; first at ... (0, 1, 0): got 16.98388671875, expected
                                            16.48388671875"
    The honest emulation passes the same check."""
    c, seed, e = R.precise_exact_cases()[2]
    assert e["res_tdiv"] == 2 and e["alpha"] == 0.5
    _exact_check(c, seed, e, None)
    msgs = {m: _first_msg(lambda: _exact_check(c, seed, e, m)) for m in ("drop_wlzh", "lo_tap", "lo_row", "lolo", "tdiv")}
    for m, s in msgs.items():
        print(m, "->", s)
        assert "elements differ" in s, (m, s)


def _staged(c, mutate=None, seed=0):
    """the emulation's staged pair of a probe case against check_staged's rule -> the assertion of the GPU test"""
    o = R.px_make_ops(c, seed)
    adain, act, slope, exact = R.PX_PRO[c.pro]
    sc, sh = R.px_consts(o)
    w = R.delta_weights(c.Co, c.Ci, c.k, 0, 0)
    S = R.x3_emulate(o["x"], w, sc=sc, sh=sh, act=act, slope=slope, snake_alpha=o["alpha"], pad=R.px_pad(c), dil=c.dil,
                     order="blk32", mutate=mutate)[1]
    if exact:
        d = first_diff(S, R.x3_identity_expect(o["x"], sc, sh, act, slope))
        assert d is None, f"the read-out differs from hi + lo of the exact prologue: {d}"
        return 0.0
    sc64, sh64 = R.adain_consts(*(o[n] for n in ("mean", "rstd", "gamma", "beta")))
    s, _, mag = pro_ref64(o["x"], sc64, sh64, act, slope, o["alpha"])
    ratio = R.x3_staged_ratio(S, s, mag)
    assert ratio <= 1, f"staged pair off by {ratio:.3f} of the per-element bound"
    return ratio


def test_mutations_turn_the_staged_check_red():
    """prologue mistakes against the identity probes' rule, with the first message of each:
      AdaIN constants of utterance 0 used for utterance 1 (130 -> 64, power-of-two AdaIN + LeakyReLU 1/8)
          -> "the read-out differs from hi + lo of the exact prologue: 560 elements differ; first at (utterance, row,
              column) (1, 0, 0): got -0.1817612648010254, expected -0.7270450592041016"
      Snake alpha of channel c & 127 (256 -> 256)
          -> "staged pair off by 187758.709 of the per-element bound"
    The honest emulation (torch's fp32 sine, two roundings in the affine) stays below 1: largest ratio 0.8832."""
    ca = R.PxCase("conv", 2, 5, 130, 64, 3, 1, "adain2_leaky8", 128)
    cs = R.PxCase("conv", 2, 65, 256, 256, 3, 1, "snake", 128)
    assert _staged(ca) == 0.0
    r = max(_staged(cs), _staged(R.PxCase("conv", 2, 129, 130, 64, 3, 1, "adain_leaky.2", 128)))
    print(f"honest emulation: staged max ratio {r:.4f}")
    m1 = _first_msg(lambda: _staged(ca, "adain_utt0"))
    m2 = _first_msg(lambda: _staged(cs, "alpha127"))
    print(m1, "\n", m2)
    assert "differs from hi + lo of the exact prologue" in m1 and "(1, " in m1
    assert "of the per-element bound" in m2


@pytest.mark.parametrize("case", [v for v in R.precise_dense_cases() if not v[0].ups], ids=R.px_dense_id)
def test_dense_ratio_holds_on_the_honest_emulation(case):
    """x3_dense_ratio <= 1 for the emulation of every dense case of the GPU table (blocked order; T cut to 40 rows and
    Co to 32 channels: the bound is per element), against ref_full = sum w S on the emulation's own staged pair (the polyphase ConvTranspose case is not emulated).  A
    per-element bound on random operands cannot see one lo fragment: with wl zh dropped in a K-step the ratio on the
    first case is 0.34, with a lo row displaced 0.86 (printed) -- those mistakes are what the exact-sum check is for."""
    c, e = case
    c = c._replace(T=40, Co=min(c.Co, 32))
    o, d = R.px_make_ops(c, 0), R.px_dense_operands(c, e)
    adain, act, slope, _ = R.PX_PRO[c.pro]
    sc, sh = R.px_consts(o)
    kw = dict(sc=sc, sh=sh, act=act, slope=slope, snake_alpha=o["alpha"], pad=R.px_pad(c), dil=c.dil, stride=c.stride, res=d["res"],
              res_tdiv=e["res_tdiv"], out_scale=e["alpha"], acc_in=d["acc"], beta=e["beta"], gate=d["gate"], order="blk32")
    y, S = R.x3_emulate(o["x"], d["w"], d["b"], **kw)
    ref, terms, K = R.px_dense_ref(c, S, d, e)
    ratio = R.x3_dense_ratio(y, ref, terms, K)
    assert ratio <= 1, ratio
    if c.k == 7 and not e["res"] and not e["acc"] and e["alpha"] == 1.0:
        for m in ("drop_wlzh", "lo_row"):
            ym, _ = R.x3_emulate(o["x"], d["w"], d["b"], **dict(kw, mutate=m))
            print(m, R.x3_dense_ratio(ym, ref, terms, K))
