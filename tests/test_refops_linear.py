"""CPU self-checks of the linears' references and probe helpers in tests/refops.py (used by
tests/test_gpu_linear_probe.py): the helpers against direct computation, the identity probe and the per-element bounds
on an honest fp32 emulation of the GEMM kernels (K-step by K-step, slices summed in order, the fused epilogue, one
rounding of the output), and the same checks going red on emulations with one mistake each -- a dropped K-step, a
duplicated one, a K-step a split slice adds twice, a clamped row written instead of skipped, the gate of the
neighbouring utterance, a column scale shifted by one, column Co stored."""
import math

import pytest
import torch

from refops import (LIN_SENT, LinCase, act_ratio, bf, conv_terms_ref, delta_weights, dense_ratio, e4m3_case, e4m3_value,
                    fill_bits, first_diff, gemm_tile128_rows, gemm_tile_rows, layernorm_image_ok, layernorm_ref64,
                    lin_ci_pad, lin_expected_launch, lin_id, linear_cases, linear_probe_expect, quant_rows_ref, same_bits)

B, T = 3, 43  # 129 rows: a 64-row tile spans two utterances


def emu(xs, w, b=None, *, SK=1, ks=32, gate=None, res=None, alpha=1.0, acc_in=None, beta=0.0, sx=None, sw=None,
        act=None, out_dt=torch.bfloat16, mut=None):
    """the GEMM kernels in fp32 on staged operands xs [B, T, K] and weights w [Co, K] (K a multiple of ks, zero padded):
    slice z accumulates its K-steps in order, the slices are summed in order, fp8: acc (sx sw); then act(. + bias), the
    gate of the row's utterance, + residual, alpha, + beta acc_in, one rounding to out_dt -> [B T, Co (+ 1)].
    mut: "drop" | "dup" | "twice" | "gate" | "scale" | "co" (module docstring; "co" appends the stored column Co)"""
    Bn, Tn, K = xs.shape
    X = xs.reshape(Bn * Tn, K).float()
    nks = K // ks // SK
    parts = []
    for z in range(SK):
        steps = list(range(z * nks, (z + 1) * nks))
        if mut == "drop" and z == SK - 1:
            steps = steps[:-1]
        if mut == "dup" and z == 0:
            steps = steps + steps[-1:]
        if mut == "twice" and z > 0:
            steps = [steps[0] - 1] + steps
        acc = torch.zeros(Bn * Tn, w.shape[0])
        for k in steps:
            acc = acc + X[:, k * ks:(k + 1) * ks] @ w[:, k * ks:(k + 1) * ks].float().t()
        parts.append(acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    if sx is not None:
        acc = acc * (sx[:, None] * (sw.roll(-1) if mut == "scale" else sw)[None, :])
    v = acc + (b.float() if b is not None else 0.0)
    if act == "gelu":
        v = torch.nn.functional.gelu(v)
    rows = torch.arange(Bn * Tn)
    if gate is not None:
        utt = (rows // 64 * 64 if mut == "gate" else rows) // Tn  # ("gate": the utterance of the tile's first row)
        v = v * gate.float()[utt]
    if res is not None:
        v = v + res.reshape(Bn * Tn, -1).float()
    v = v * alpha
    if acc_in is not None:
        v = v + beta * acc_in.reshape(Bn * Tn, -1).float()
    if mut == "co":
        v = torch.cat([v, v[:, -1:]], 1)
    return v.to(out_dt)


def stored(y, Bn, Tn, Co, dt, mut=None):
    """the emulated stores into a sentinel-filled buffer [B + 2, T + 2, 8 + ceil8(Co) + 8] at channel offset 8 (the last
    two utterances are guard only) -> (buffer, the sentinel image of it with the logical region cut out the same way).
    mut "clamp": the rows of the last 64-row tile past B T are written (at their unclamped addresses) instead of skipped"""
    ld = 8 + (Co + 7) // 8 * 8 + 8
    buf = fill_bits((Bn + 2, Tn + 2, ld), dt, LIN_SENT[dt])
    want = buf.clone()
    M = Bn * Tn
    rows = list(range(M)) + (list(range(M, (M + 63) // 64 * 64)) if mut == "clamp" else [])
    for R in rows:
        src = min(R, M - 1)
        buf[R // Tn, R % Tn, 8:8 + y.shape[1]] = y[src]
    want[:Bn, :Tn, 8:8 + Co] = buf[:Bn, :Tn, 8:8 + Co]
    return buf, want


def operands(K, Co, seed=0):
    g = torch.Generator().manual_seed(seed + K + Co)
    x = bf(torch.randn(B, T, K, generator=g))
    w = bf(torch.randn(Co, K, generator=g) / math.sqrt(K))
    b = torch.randn(Co, generator=g) * 0.1
    gate = torch.rand(B, Co, generator=g) + 0.5
    res = torch.randn(B, T, Co, generator=g)
    return x, w, b, gate, res


def identity_problem(K, Co, SK, mut, out_dt=torch.float32):
    """the GPU file's identity assertions on the emulation -> the first failing one's message, or None"""
    x = operands(K, Co)[0]
    for m in range((K + Co - 1) // Co if Co < K else 1):
        y = emu(x, delta_weights(Co, K, 1, 0, m)[:, :, 0], SK=SK, out_dt=out_dt, mut=mut)
        buf, want = stored(y, B, T, Co, out_dt, mut)
        if not same_bits(buf, want):
            return "a y guard was overwritten"
        d = first_diff(buf[:B, :T, 8:8 + Co], linear_probe_expect(x.to(out_dt), Co, m))
        if d is not None:
            return "the output is not the staged operand: " + d
    return None


@pytest.mark.parametrize("K,Co,SK", [(128, 200, 1), (384, 200, 4), (384, 80, 2), (64, 22, 2), (512, 16, 1)])
def test_identity_probe_passes_on_the_honest_emulation(K, Co, SK):
    assert identity_problem(K, Co, SK, None) is None
    assert identity_problem(K, Co, SK, None, torch.bfloat16) is None


@pytest.mark.parametrize("mut,K,Co,SK,word", [("drop", 128, 200, 1, "staged operand"), ("drop", 384, 80, 2, "staged operand"),
                                              ("dup", 128, 200, 1, "staged operand"), ("dup", 64, 22, 2, "staged operand"),
                                              ("twice", 384, 200, 4, "staged operand"), ("twice", 64, 22, 2, "staged operand"),
                                              ("clamp", 128, 200, 1, "guard"), ("co", 128, 200, 1, "guard"),
                                              ("co", 64, 22, 2, "guard")])
def test_identity_probe_bites(mut, K, Co, SK, word):
    msg = identity_problem(K, Co, SK, mut)
    assert msg is not None and word in msg, msg


def dense_figure(mut, SK=1, out_dt=torch.float32, act=None):
    K, Co = 384, 200
    x, w, b, gate, res = operands(K, Co, 1)
    gated = act is None
    y = emu(x, w, b, SK=SK, gate=gate if gated else None, res=res if gated else None, alpha=0.75, act=act, out_dt=out_dt,
            mut=mut)
    z, terms = conv_terms_ref(x, w[:, :, None], b, gate=gate if gated else None, res=res if gated else None,
                              out_scale=1.0 if act else 0.75)
    got = y.view(B, T, -1)[:, :, :Co]
    if act:
        return act_ratio(got / 0.75, z, terms, K + SK - 1, act, out_dt == torch.bfloat16)
    return dense_ratio(got, z, terms, K + SK - 1, out_dt == torch.bfloat16)


@pytest.mark.parametrize("out_dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("SK", [1, 4])
def test_dense_bound_holds_on_the_honest_emulation(SK, out_dt):
    assert dense_figure(None, SK, out_dt) <= 1
    assert dense_figure(None, SK, torch.float32, "gelu") <= 1


@pytest.mark.parametrize("mut,SK", [("drop", 1), ("dup", 1), ("twice", 4), ("gate", 1), ("gate", 4)])
def test_dense_bound_bites(mut, SK):
    assert dense_figure(mut, SK) > 1
    assert dense_figure(mut, SK, torch.bfloat16) > 1
    if mut != "gate":
        assert dense_figure(mut, SK, torch.float32, "gelu") > 1


def test_conv_terms_ref_gate():
    x, w, b, gate, res = operands(128, 80, 2)
    y, terms = conv_terms_ref(x, w[:, :, None], b, gate=gate, res=res, out_scale=0.5)
    want = ((x.double() @ w.double().t() + b.double()) * gate.double()[:, None, :] + res.double()) * 0.5
    assert torch.allclose(y, want, rtol=1e-13, atol=1e-13)
    wt = ((x.double().abs() @ w.double().abs().t() + b.double().abs()) * gate.double()[:, None, :] + res.double().abs()) * 0.5
    assert torch.allclose(terms, wt, rtol=1e-13, atol=1e-13)
    assert torch.equal(conv_terms_ref(x, w[:, :, None], b)[0], conv_terms_ref(x, w[:, :, None], b, gate=None)[0])


def test_fp8_case_and_column_scale():
    """the e4m3 case holds every special code and no NaN, its scales are distinct powers of two, the expected identity
    output code x 448 x scale is exact in bf16; a column scale shifted by one fails the dense bound (the identity
    probe's scales are all 1: it cannot see it)"""
    from stzs.weights import quantize_f8_cols
    codes, sx = e4m3_case(B, T, 128)
    assert not bool(((codes & 0x7F) == 0x7F).any())
    for s in (0x00, 0x80, 0x01, 0x81, 0x07, 0x87, 0x7E, 0xFE):
        assert bool((codes == s).any(-1).all()), hex(s)
    assert len(set(sx.tolist())) == B * T and bool((torch.frexp(sx)[0] == 0.5).all())
    v = e4m3_value(codes) * sx.view(B, T, 1) * 448.0
    assert bool(torch.isfinite(v).all()) and torch.equal(v.to(torch.bfloat16).float(), v)
    q, sc = quantize_f8_cols(delta_weights(200, 128, 1, 0)[:, :, 0] * 448.0)
    assert bool((sc == 1.0).all()) and float(q.float().max()) == 448.0
    y = emu(e4m3_value(codes), q.float(), ks=64, sx=sx, sw=sc, out_dt=torch.float32)
    assert first_diff(y.view(B, T, -1), linear_probe_expect(v + 0.0, 200)) is None
    # dense, real scales
    g = torch.Generator().manual_seed(5)
    xr = torch.randn(B, T, 320, generator=g) * torch.rand(B, T, 1, generator=g) * 4
    cx, sxr = quant_rows_ref(xr)
    w = torch.randn(200, 320, generator=g) / math.sqrt(320) * (torch.rand(200, 1, generator=g) + 0.5)
    qw, sw = quantize_f8_cols(w)
    z, terms = conv_terms_ref(e4m3_value(cx) * sxr[..., None], (qw.float() * sw[:, None])[:, :, None], None)
    for mut, ok in ((None, True), ("scale", False)):
        y = emu(e4m3_value(cx), qw.float(), ks=64, sx=sxr.reshape(-1), sw=sw, out_dt=torch.float32, mut=mut)
        assert (dense_ratio(y.view(B, T, -1), z, terms, 320 + 2, False) <= 1) == ok, mut


def test_tile_rule_and_table():
    assert gemm_tile_rows(3200, 2048, 256) == 128 and gemm_tile_rows(3137, 2048, 256) == 128
    assert gemm_tile_rows(3072, 2048, 256) == 64 and gemm_tile_rows(129, 256, 256) == 64
    assert gemm_tile128_rows(256) == 3200 and gemm_tile128_rows(10 ** 6) is None
    cases = linear_cases(256)
    assert len({lin_id(c) for c in cases}) == len(cases)
    for c in cases:
        assert lin_ci_pad(c) >= c.Ci and lin_expected_launch(c)[3] == max(c.Z, 1)
    assert not any(c.kern == "glds128" for c in linear_cases(10 ** 6))
    # every K-step count per slice the issue names is in the table: 1, 2, 3, 6 (split), 1, 2, 4, 12 (unsplit)
    per = {(c.Z, lin_ci_pad(c) // 32 // max(c.Z, 1)) for c in cases if c.kern == "glds"}
    assert {(2, 1), (2, 2), (4, 1), (4, 3), (2, 6), (0, 1), (0, 2), (0, 4), (0, 12)} <= per


def test_layernorm_rule_bites():
    """an fp32 LayerNorm rounded to bf16 passes test_row_layernorm_edges' rule against the fp64 reference; the modulation
    of the neighbouring utterance, or a variance without eps, does not"""
    g = torch.Generator().manual_seed(3)
    R, K = 129, 256
    x = torch.randn(R, K, generator=g) * 2 + 0.3
    G, Bt = torch.randn(3, K, generator=g) * 0.2, torch.randn(3, K, generator=g) * 0.1
    grp = torch.arange(R) // 43
    ref, terms = layernorm_ref64(x, G, Bt, grp, 1.0)

    def f32(gr, eps=1e-5):
        mu = x.mean(1, keepdim=True)
        rs = 1 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
        return ((x - mu) * rs * (1 + G[gr]) + Bt[gr]).to(torch.bfloat16)
    assert layernorm_image_ok(f32(grp), ref, terms)[0]
    assert not layernorm_image_ok(f32((torch.arange(R) // 16 * 16) // 43), ref, terms)[0]
    assert not layernorm_image_ok(f32(grp, eps=1e-2), ref, terms)[0]
