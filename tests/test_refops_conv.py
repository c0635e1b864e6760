"""CPU self-checks of the conv-family references and probe helpers in tests/refops.py (used by
tests/test_gpu_conv_probe.py): the fp64 references against torch's own convolutions, the delta-weight identity and the
per-element bounds on an honest fp32 emulation of the kernels (bf16(pro(x)) -> conv -> bf16), and the same checks going
red on emulations with one staging or addressing mistake each."""
import math

import pytest
import torch
import torch.nn.functional as F

from refops import (adain_consts, bf, conv_terms_ref, delta_weights, delta_weights_T, dense_ratio, polyphase_expect,
                    pro_ref64, probe_readout, probe_readout_T, round_bf16, staged_check)

# (B, T, Ci, Co, k, dil): three of the GPU probe's shapes -- single chunk, multi-chunk with Ci > Co, ragged tiles
SHAPES = [(2, 200, 128, 128, 3, 5), (2, 129, 256, 256, 7, 3), (2, 65, 384, 176, 11, 5)]


def _operands(shape, seed=0):
    B, T, Ci, Co, k, dil = shape
    g = torch.Generator().manual_seed(seed + T + Ci + k)
    x = bf(torch.randn(B, T, Ci, generator=g))
    mean = torch.randn(B, Ci, generator=g) * 0.1
    rstd = torch.rand(B, Ci, generator=g) + 0.5
    gamma, beta = torch.randn(B, Ci, generator=g) * 0.2, torch.randn(B, Ci, generator=g) * 0.2
    alpha = torch.exp(torch.empty(Ci).uniform_(math.log(0.25), math.log(4.0), generator=g))
    w = bf(torch.randn(Co, Ci, k, generator=g) / math.sqrt(Ci * k))
    b = torch.randn(Co, generator=g) * 0.1
    res = bf(torch.randn(B, T, Co, generator=g))
    return x, mean, rstd, gamma, beta, alpha, w, b, res


def emu_stage(x, mean, rstd, gamma, beta, alpha, mut=None):
    """the kernels' staging in fp32: AdaIN constants, Snake, one rounding to bf16"""
    sc = (1 + gamma) * rstd
    sh = beta - mean * sc
    al = alpha.clone()
    if mut == "alpha":  # one channel takes its neighbour's alpha
        al[5] = alpha[6]
    if mut == "shift":  # the shift of the neighbouring utterance
        sh = sh.roll(1, 0)
    v = x * sc[:, None, :] + sh[:, None, :]
    return (v + torch.sin(al * v) ** 2 / al).to(torch.bfloat16)


def emu_conv(staged, w, b, k, dil, res=None, out_scale=1.0, mut=None):
    """tile by tile, as the kernels run: 64 output rows from 64 + (k - 1) dil staged rows (zero padded), fp32
    accumulation, one rounding to bf16"""
    B, T, Ci = staged.shape
    pad = dil * (k - 1) // 2
    xp = F.pad(staged.float(), (0, 0, pad, pad + 64))
    w = w.clone()
    if mut == "drop":  # one (input channel, tap) never accumulated
        w[:, 17, k - 1] = 0
    out = []
    for t0 in range(0, T, 64):
        tile = xp[:, t0:t0 + 64 + (k - 1) * dil].clone()
        if mut == "halo":  # the last halo row of every tile is stale in the last 8 channels
            tile[:, -1, -8:] = tile[:, -2, -8:]
        out.append(F.conv1d(tile.transpose(1, 2), w, b, dilation=dil).transpose(1, 2))
    y = torch.cat(out, 1)[:, :T]
    if res is not None:
        y = y + res
    return (y * out_scale).to(torch.bfloat16)


def _checks(shape, mut=None):
    """the GPU file's probe and dense checks on the emulation -> (probe problems, staged ratio, staged share of
    differing bits, dense ratio)"""
    B, T, Ci, Co, k, dil = shape
    x, mean, rstd, gamma, beta, alpha, w, b, res = _operands(shape)
    pad = dil * (k - 1) // 2
    staged = emu_stage(x, mean, rstd, gamma, beta, alpha, mut)
    run = lambda j0, m: emu_conv(staged, delta_weights(Co, Ci, k, j0, m), None, k, dil, mut=mut)
    S, problems = probe_readout(run, T=T, Ci=Ci, Co=Co, k=k, dil=dil, pad=pad)
    sc, sh = adain_consts(mean, rstd, gamma, beta)
    s, sbf, mag = pro_ref64(x, sc, sh, "snake", alpha=alpha)
    ratio, share = staged_check(S, s, sbf, mag)
    got = emu_conv(staged, w, b, k, dil, res=res, out_scale=0.7071, mut=mut)
    ref, terms = conv_terms_ref(S.float(), w, b, pad=pad, dil=dil, res=res, out_scale=0.7071)
    return problems, ratio, share, dense_ratio(got, ref, terms, Ci * k, True), torch.equal(S, staged)


def test_round_bf16_is_one_rounding():
    """2^-9 above a bf16 tie rounds up in one step; through fp32 (torch's conversion) the tie is hit and goes to even"""
    s = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8, -3.0, 0.0, 0.1], dtype=torch.float64)
    r = round_bf16(s).double()
    assert r[0].item() == 1.0 + 2.0 ** -7 and r[1].item() == 1.0 and r[2].item() == -3.0 and r[3].item() == 0.0
    assert abs(r[4].item() - 0.1) <= 0.1 * 2.0 ** -9
    assert s[0].float().to(torch.bfloat16).item() == 1.0  # the double rounding the helper avoids


@pytest.mark.parametrize("stride,dil,k,pad,tdiv", [(1, 1, 3, 1, 1), (1, 5, 11, 25, 2), (6, 1, 12, 3, 1)])
def test_conv_terms_ref_vs_torch(stride, dil, k, pad, tdiv):
    g = torch.Generator().manual_seed(k)
    B, T, Ci, Co = 2, 77, 24, 16
    x = torch.randn(B, T, Ci, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, k, generator=g, dtype=torch.float64)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    y0 = F.conv1d(x.transpose(1, 2), w, b, stride=stride, padding=pad, dilation=dil).transpose(1, 2)
    To = y0.shape[1]
    res = torch.randn(B, (To + tdiv - 1) // tdiv, Co, generator=g, dtype=torch.float64)
    acc = torch.randn(B, To, Co, generator=g, dtype=torch.float64)
    y, terms = conv_terms_ref(x, w, b, pad=pad, dil=dil, stride=stride, res=res, res_tdiv=tdiv, out_scale=-0.5,
                              acc_in=acc, beta=-2.0)
    r = res.repeat_interleave(tdiv, 1)[:, :To]
    assert torch.allclose(y, (y0 + r) * -0.5 - 2.0 * acc, rtol=0, atol=1e-12)
    t0 = F.conv1d(x.abs().transpose(1, 2), w.abs(), b.abs(), stride=stride, padding=pad, dilation=dil).transpose(1, 2)
    assert torch.allclose(terms, (t0 + r.abs()) * 0.5 + 2.0 * acc.abs(), rtol=0, atol=1e-12)
    assert (terms >= y.abs() - 1e-12).all()


@pytest.mark.parametrize("s,refl", [(4, 1), (6, 0), (10, 1)])
def test_polyphase_refs_vs_torch(s, refl):
    """conv_terms_ref's ConvTranspose form, and polyphase_expect / delta_weights_T, against F.conv_transpose1d"""
    g = torch.Generator().manual_seed(s)
    B, T, Ci, Co = 2, 9, 12, 8
    x = torch.randn(B, T, Ci, generator=g, dtype=torch.float64)
    w = torch.randn(Ci, Co, 2 * s, generator=g, dtype=torch.float64)
    y, _ = conv_terms_ref(x, w, None, ups=s, ups_pad=s // 2, refl=refl)
    y0 = F.conv_transpose1d(x.transpose(1, 2), w, None, stride=s, padding=s // 2)
    y0 = (F.pad(y0, (1, 0), mode="reflect") if refl else y0).transpose(1, 2)
    assert y.shape == (B, T * s + refl, Co) and torch.equal(y, y0)
    for j0 in range(2 * s):
        for m in range(2):
            d, _ = conv_terms_ref(x, delta_weights_T(Ci, Co, 2 * s, j0, m).double(), None, ups=s, ups_pad=s // 2, refl=refl)
            blk = torch.zeros(B, T, Co, dtype=torch.float64)
            blk[:, :, :min(Co, Ci - m * Co)] = x[:, :, m * Co:(m + 1) * Co]
            assert torch.equal(d, polyphase_expect(blk, j0, ups=s, ups_pad=s // 2, refl=refl))
    run = lambda j0, m: conv_terms_ref(x, delta_weights_T(Ci, Co, 2 * s, j0, m).double(), None, ups=s, ups_pad=s // 2,
                                       refl=refl)[0].float()
    S, problems = probe_readout_T(run, T=T, Ci=Ci, Co=Co, ups=s, ups_pad=s // 2, refl=refl)
    assert not problems and torch.equal(S, x.float())


def test_pro_ref64_and_delta_weights():
    g = torch.Generator().manual_seed(1)
    x = bf(torch.randn(2, 9, 12, generator=g))
    sc, sh = torch.randn(2, 12, generator=g).double(), torch.randn(2, 12, generator=g).double()
    al = torch.rand(12, generator=g) + 0.5
    v = x.double() * sc[:, None] + sh[:, None]
    s, sbf, mag = pro_ref64(x, sc, sh, "snake", alpha=al)
    assert torch.allclose(s, v + torch.sin(al.double() * v) ** 2 / al.double(), rtol=0, atol=1e-15)
    assert torch.equal(mag, (x.double() * sc[:, None]).abs() + sh.abs()[:, None] + 1 / al.double())
    assert ((sbf.double() - s).abs() <= s.abs() * 2.0 ** -8).all()
    s, sbf, mag = pro_ref64(x, None, None, "leaky", slope=0.125)
    assert torch.equal(s, F.leaky_relu(x.double(), 0.125)) and torch.equal(sbf.double(), s) and torch.equal(mag, x.double().abs())
    w = delta_weights(8, 12, 3, 2, 1)
    assert w.sum() == 4 and all(w[c, c + 8, 2] == 1 for c in range(4))


@pytest.mark.parametrize("shape", SHAPES)
def test_emulation_passes(shape):
    """the honest emulation: the probe reads its staged tensor back bit for bit, the staged values pass the
    inexact-prologue checks and the output the bf16 per-element bound"""
    problems, ratio, share, dense, same = _checks(shape)
    print(shape, "staged ratio", ratio, "share", share, "dense ratio", dense)
    assert not problems, problems
    assert same
    assert ratio <= 1 and share <= 0.01
    assert dense <= 1


@pytest.mark.parametrize("mut", ["alpha", "shift", "halo", "drop"])
def test_mutated_emulations_fail(mut):
    """one mistake each: a channel with another channel's alpha and the neighbouring utterance's shift fail the
    per-element staged check; a stale halo row and a dropped (channel, tap) fail the probe's bit comparison -- the
    dropped one and the shift also the dense bound"""
    shape = SHAPES[1]
    problems, ratio, share, dense, _ = _checks(shape, mut)
    print(mut, problems[:2], "staged ratio", ratio, "share", share, "dense ratio", dense)
    if mut in ("alpha", "shift"):
        assert ratio > 1
    if mut in ("halo", "drop"):
        assert problems
    if mut == "drop":
        assert dense > 1
    assert problems or ratio > 1 or share > 0.01 or dense > 1
