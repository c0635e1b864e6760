"""Plain-torch fp32 restatements of the C-ABI op semantics (include/stzs.h), used as the numerics
reference for the HIP kernels.  Inputs are pre-rounded to bf16 where the kernel stores bf16, so
the kernel-vs-reference difference is only accumulation order and the output rounding."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def bf(x):
    return x.to(torch.bfloat16).float()


def act(x, kind, slope=0.0, alpha=None):
    if kind == "leaky":
        return F.leaky_relu(x, slope)
    if kind == "snake":
        a = alpha[None, :, None]
        return x + torch.sin(a * x) ** 2 / a
    if kind == "gelu":
        return F.gelu(x)
    if kind == "silu":
        return F.silu(x)
    return x


def conv_ref(x_ntc, w, b, *, pad=0, dil=1, stride=1, sc=None, sh=None, pro_act=None, slope=0.0, alpha=None,
             epi_act=None, gate=None, res=None, res_tdiv=1, out_scale=1.0, acc_in=None, beta=0.0):
    """x [B, T, Ci] (fp32 holding bf16 values), w [Co, Ci, k] -> [B, T_out, Co] fp32."""
    x = x_ntc.transpose(1, 2)
    if sc is not None:
        x = x * sc[:, :, None] + sh[:, :, None]
    x = act(x, pro_act, slope, alpha)
    x = bf(x)
    y = F.conv1d(x, bf(w), b, stride=stride, padding=pad, dilation=dil).transpose(1, 2)
    y = act(y, epi_act)
    if gate is not None:
        y = y * gate[:, None, :]
    if res is not None:
        r = res
        if res_tdiv > 1:
            r = r.repeat_interleave(res_tdiv, dim=1)[:, : y.shape[1]]
        y = y + r
    y = y * out_scale
    if acc_in is not None:
        y = y + beta * acc_in
    return y


def convT_ref(x_ntc, w, b, *, stride, pad, refl=0, pro_act=None, slope=0.0, res=None):
    x = bf(act(x_ntc.transpose(1, 2), pro_act, slope))
    y = F.conv_transpose1d(x, bf(w), b, stride=stride, padding=pad)
    if refl:
        y = F.pad(y, (1, 0), mode="reflect")
    y = y.transpose(1, 2)
    if res is not None:
        y = y + res
    return y


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def max_rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ---- fp64 restatements of the attention / glue kernels (tests/test_gpu_attention.py, test_gpu_glue.py) ----
# Each takes the kernel's operands as they are stored (fp32 tensors holding the stored values) and returns fp64.

def attention_ref(q, k, v, heads):
    """q [R, Lq, D], k / v [R, Lk, D] -> (softmax(q k^T / sqrt(dh)) v, softmax(q k^T / sqrt(dh)) |v|), both
    [R, Lq, D] fp64.  The second is the magnitude an output element's rounding errors scale with."""
    R, Lq, D = q.shape
    dh = D // heads
    qd, kd, vd = (t.double().reshape(R, -1, heads, dh).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qd @ kd.transpose(-1, -2) / math.sqrt(dh), -1)
    back = lambda t: t.transpose(1, 2).reshape(R, Lq, D)
    return back(p @ vd), back(p @ vd.abs())


def prprep_ref(codes, h, T, c0, Cs):
    """codes [B, L, >= c0 + Cs], h [B, T, Ch] -> [B, T, Ch + Cs] fp64: the h copy, then the linear resample
    (F.interpolate, align_corners=False) of codes[:, :, c0:c0 + Cs] from L to T rows."""
    z = F.interpolate(codes[:, :, c0:c0 + Cs].double().transpose(1, 2), size=T, mode="linear", align_corners=False)
    return torch.cat([h.double(), z.transpose(1, 2)], -1)


def dwup_ref(x, mean, rstd, gamma, beta, w, wb, slope):
    """AdaIN + LeakyReLU + depthwise ConvTranspose1d(k3, s2, p1, op1).  x [B, T, C], mean / rstd / gamma / beta
    [B, C], w [C, 3], wb [C] -> (y [B, 2T, C], terms [B, 2T, C]) fp64.  terms is the same transposed conv on
    magnitudes: sum over taps of |w| * lrelu'(v) * (|x sc| + |mu sc| + |beta|), sc = (1 + gamma) rstd, plus |bias|
    -- every product the kernel rounds is one of these pieces, so its fp32 error is a few 2^-24 of it."""
    x, mean, rstd, gamma, beta, w, wb = (t.double() for t in (x, mean, rstd, gamma, beta, w, wb))
    C = x.shape[-1]
    sc = ((1 + gamma) * rstd)[:, None, :]
    v = (1 + gamma)[:, None, :] * (x - mean[:, None, :]) * rstd[:, None, :] + beta[:, None, :]
    mag = ((x * sc).abs() + (mean[:, None, :] * sc).abs() + beta[:, None, :].abs()) * torch.where(v >= 0, 1.0, slope)
    up = lambda t, ww, bb: F.conv_transpose1d(t.transpose(1, 2), ww[:, None, :], bb, stride=2, padding=1,
                                               output_padding=1, groups=C).transpose(1, 2)
    return up(F.leaky_relu(v, slope), w, wb), up(mag, w.abs(), wb.abs())


def f0n_ref(f, w4):
    """Conv1d(1, 1, k3, s2, p1): f [B, T80], w4 = (w0, w1, w2, bias) -> (y [B, T80 / 2], sum of |terms|) fp64."""
    f, w4 = f.double(), w4.double()
    cv = lambda t, ww: F.conv1d(t[:, None, :], ww[None, None, :3], ww[3:4], stride=2, padding=1)[:, 0]
    return cv(f, w4), cv(f.abs(), w4.abs())


def dn_cond_ref(pool, temb):
    """pool [R, D], temb [steps, D] fp32 -> silu(pool + temb[s]) [steps, R, D] fp64.  The sum is the kernel's one
    fp32 addition (IEEE, exactly rounded -- part of the operation's definition); the SiLU of it is fp64."""
    x = (pool.float()[None] + temb.float()[:, None, :]).double()
    return x / (1 + torch.exp(-x))


def mean_rows_seq32(x):
    """x [B, L, C] fp32 -> [B, C] fp32 with the kernel's arithmetic: the rows added in order in fp32, one division."""
    xs = x.numpy().astype(np.float32)
    s = np.zeros((xs.shape[0], xs.shape[2]), np.float32)
    for l in range(xs.shape[1]):
        s = (s + xs[:, l]).astype(np.float32)
    return torch.from_numpy((s / np.float32(xs.shape[1])).astype(np.float32))


def adaln_expand_seq32(mod, table, D, nlayers, mask):
    """mod [R, nchunk * D], table [nlayers, nchunk * D] | None -> [nlayers, R, nchunk * D] fp32 with the kernel's
    arithmetic: (mod + table[l]) rounded to fp32, then + 1 on the chunks j / D whose bit is set in mask."""
    m = mod.numpy().astype(np.float32)
    out = np.repeat(m[None], nlayers, 0)
    if table is not None:
        out = (out + table.numpy().astype(np.float32)[:, None, :]).astype(np.float32)
    one = np.array([(mask >> (j // D)) & 1 for j in range(m.shape[1])], bool)
    out[:, :, one] = (out[:, :, one] + np.float32(1)).astype(np.float32)
    return torch.from_numpy(out)


def _ordered(t):
    """the bits of a bf16 / fp32 tensor as integers ordered like the values (+0 and -0 both 0)"""
    i = t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).long()
    mag = i & (0x7FFF if t.dtype == torch.bfloat16 else 0x7FFFFFFF)
    return torch.where(i < 0, -mag, mag)


def ulp_dist(a, b):
    """elementwise distance in units in the last place between two tensors of the same dtype (bf16 or fp32)"""
    assert a.dtype == b.dtype and a.shape == b.shape
    return (_ordered(a) - _ordered(b)).abs().view(a.shape)


def ulp_diff(a, b):
    """the largest ulp_dist (0 for empty tensors)"""
    return ulp_dist(a, b).max().item() if a.numel() else 0


def same_bits(a, b):
    """bit-for-bit equality (distinguishes -0 from +0, equates identical NaNs)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    vt = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(vt), b.contiguous().view(vt))
