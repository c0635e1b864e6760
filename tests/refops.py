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
    vt = {1: torch.int8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(vt), b.contiguous().view(vt))


# ---- conv family: staged-operand probes and per-element bounds (tests/test_gpu_conv_probe.py, test_refops_conv.py) ----
# The conv kernels stage pro(x) as bf16 and feed it to MFMA.  With a one-hot weight (delta_weights), bias 0, no residual,
# alpha 1, every output is one staged value plus products 0 * finite: the launch reads the staged tensor out bit for bit.

def round_bf16(s):
    """fp64 -> bf16 with ONE rounding (nearest even on 8 significant bits); torch's double -> bfloat16 rounds to fp32
    first.  Normal range only (the probes' magnitudes)."""
    m, e = torch.frexp(s.double())
    return torch.ldexp(torch.round(m * 256.0), e - 8).to(torch.bfloat16)


def adain_consts(mean, rstd, gamma, beta):
    """-> (sc, sh) fp64 [B, C] of the AdaIN prologue: sc = (1 + gamma) rstd, sh = beta - mean sc"""
    sc = (1 + gamma.double()) * rstd.double()
    return sc, beta.double() - mean.double() * sc


def pro_ref64(x, sc=None, sh=None, act=None, slope=0.0, alpha=None):
    """the conv prologue in fp64.  x [B, T, C] (stored values), sc / sh [B, C] | None (1, 0), act None | "leaky" |
    "snake" (v + sin^2(alpha v) / alpha, alpha [C]) -> (s fp64, its bf16 rounding -- one rounding from fp64 --, the
    magnitude |x sc| + |sh| (+ 1 / alpha for Snake) that the fp32 prologue's rounding errors scale with)."""
    x = x.double()
    v, mag = x, x.abs()
    if sc is not None:
        v = x * sc.double()[:, None, :] + sh.double()[:, None, :]
        mag = (x * sc.double()[:, None, :]).abs() + sh.double().abs()[:, None, :]
    if act == "leaky":
        s = torch.where(v >= 0, v, v * slope)
    elif act == "snake":
        a = alpha.double()[None, None, :]
        s = v + torch.sin(a * v) ** 2 / a
        mag = mag + 1 / a
    else:
        assert act is None, act
        s = v
    return s, round_bf16(s), mag


def staged_check(got, s, sbf, mag):
    """a staged bf16 tensor against pro_ref64's (s, sbf, mag) -> (the largest |got - s| / (2^-8 |s| + 2^-16 mag), the
    share of elements whose bits differ from sbf).  The first must be <= 1, the second <= 0.01."""
    ratio = (got.double() - s).abs() / (s.abs() * 2.0 ** -8 + mag * 2.0 ** -16)
    diff = got.contiguous().view(torch.int16) != sbf.contiguous().view(torch.int16)
    return ratio.max().item(), diff.double().mean().item()


def conv_terms_ref(xhat, w, b, *, pad=0, dil=1, stride=1, res=None, res_tdiv=1, out_scale=1.0, acc_in=None, beta=0.0,
                   ups=0, ups_pad=0, refl=0, gate=None):
    """conv_ref / convT_ref on already-staged operands, in fp64, with the magnitude its rounding errors scale with.
    xhat [B, T, Ci] (the staged values), w [Co, Ci, k] (ups > 0: ConvTranspose1d weights [Ci, Co, 2 ups], stride ups,
    padding ups_pad, ReflectionPad(refl, 0)) as the kernel holds them (bf16-rounded by the caller), b [Co] | None ->
    (y, terms) [B, T_out, Co] fp64; terms is the same conv on |xhat|, |w|, |b|, plus |res| and |beta acc_in|.
    gate [B, Co] | None: the per-utterance DiT gate of the linears, on conv + bias and before the residual
    (include/stzs.h: y = ((W x + b) gate[utterance] + res) alpha + beta acc_in); terms takes |gate|."""
    def run(x, ww, bb, r, a, gt):
        x = x.double().transpose(1, 2)
        bb = bb.double() if bb is not None else None
        if ups:
            y = F.conv_transpose1d(x, ww.double(), bb, stride=ups, padding=ups_pad)
            if refl:
                y = F.pad(y, (refl, 0), mode="reflect")
        else:
            y = F.conv1d(x, ww.double(), bb, stride=stride, padding=pad, dilation=dil)
        y = y.transpose(1, 2)
        if gt is not None:
            y = y * gt.double()[:, None, :]
        if r is not None:
            r = r.double()
            if res_tdiv > 1:
                r = r.repeat_interleave(res_tdiv, dim=1)[:, : y.shape[1]]
            y = y + r
        y = y * out_scale
        if a is not None:
            y = y + beta * a.double()
        return y
    ab = lambda t: t.abs() if t is not None else None
    y = run(xhat, w, b, res, acc_in, gate)
    out_scale, beta = abs(out_scale), abs(beta)
    return y, run(xhat.abs(), w.abs(), ab(b), ab(res), ab(acc_in), ab(gate))


def dense_ratio(got, ref, terms, K, bf16_out):
    """the largest |got - ref| / bound, bound = (2^-8 |ref| if the output is bf16) + 2 (K + 4) 2^-24 terms: one output
    rounding plus K fp32 accumulation steps (and the epilogue's four), the factor 2 for accumulation that is not
    round-to-nearest inside an MFMA block.  Must be <= 1."""
    bound = 2.0 * (K + 4) * 2.0 ** -24 * terms
    if bf16_out:
        bound = bound + ref.abs() * 2.0 ** -8
    return ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


def delta_weights(Co, Ci, k, j0, m=0):
    """one-hot conv weight [Co, Ci, k]: w[co, ci, j] = 1 where ci == co + m Co and j == j0 -- output channel co reads
    out staged channel co + m Co at tap j0 (exactly 0 where co + m Co >= Ci)"""
    w = torch.zeros(Co, Ci, k)
    n = min(Co, Ci - m * Co)
    if n > 0:
        i = torch.arange(n)
        w[i, i + m * Co, j0] = 1.0
    return w


def delta_weights_T(Ci, Co, k, j0, m=0):
    """the ConvTranspose1d twin [Ci, Co, k]: w[ci, co, j] = 1 where ci == co + m Co and j == j0"""
    return delta_weights(Co, Ci, k, j0, m).transpose(0, 1).contiguous()


def fill_bits(shape, dtype, fill, device="cpu"):
    """a tensor of `dtype` filled with `fill`: a float value, or an int bit pattern (e.g. a NaN payload)"""
    if isinstance(fill, int):
        it = {1: torch.int8, 2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]
        bits = fill - (1 << (8 * it.itemsize)) if fill >= 1 << (8 * it.itemsize - 1) else fill
        return torch.full(shape, bits, dtype=it, device=device).view(dtype)
    return torch.full(shape, fill, dtype=dtype, device=device)


def guarded(shape_logical, pads, fill, dtype=torch.bfloat16, device="cpu"):
    """an over-allocated buffer around a logical [B, T, C] tensor.  pads = (extra rows per utterance, channel offset
    c0, extra columns behind ceil8(C)); every element starts as `fill` (fill_bits) -> (buf [B, T + rows, c0 + ceil8(C) +
    cols], the engine Act over buf[:, :T] at channels [c0, c0 + C): its batch stride is the buffer's)."""
    from stzs.engine import Act
    B, T, Cc = shape_logical
    rows, c0, cols = pads
    buf = fill_bits((B, T + rows, c0 + (Cc + 7) // 8 * 8 + cols), dtype, fill, device)
    return buf, Act(buf[:, :T], c0, Cc)


def guards_intact(buf, view, fill, C=None):
    """everything of buf (from guarded, with the same `fill`) outside view's [B, T, C] still holds the fill, bit for
    bit.  C: the written width where it differs from view.C (a form that stores whole 8-column vectors)."""
    C = view.C if C is None else C
    probe = buf.clone()
    fill = fill_bits(buf.shape, buf.dtype, fill, buf.device)
    probe[:, :view.T, view.c0:view.c0 + C] = fill[:, :view.T, view.c0:view.c0 + C]
    return same_bits(probe, fill)


def _bits(t):
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _first(mask):
    """the first True index of a mask, as a tuple (for a failure message)"""
    return tuple(int(v) for v in mask.nonzero()[0])


def probe_readout(run, *, T, Ci, Co, k, dil=1, pad=0, stride=1, tile=64):
    """read a conv's staged operand out through delta weights.  run(j0, m) launches the conv with delta_weights(Co, Ci,
    k, j0, m), bias 0, no residual, alpha 1 and returns y [B, T_out, Co]: y[b, t, co] must be the staged value
    S[b, t stride + j0 dil - pad, co + m Co], or exactly +0 in the zero padding and where co + m Co >= Ci.
    -> (S [B, T, Ci] in y's dtype, problems): problems lists, with (tap, utterance, row, tile row, channel), every tap
    whose padding is not +0 or whose rows differ in bits from the same rows read through an earlier tap, and the rows
    no tap reached."""
    nb = (Ci + Co - 1) // Co
    S, filled, problems = None, None, []
    for j0 in range(k):
        y = torch.cat([run(j0, m) for m in range(nb)], -1)
        dev = y.device
        if S is None:
            S = torch.zeros(y.shape[0], T, Ci, dtype=y.dtype, device=dev)
            filled = torch.zeros(T, dtype=torch.bool, device=dev)
        bad = _bits(y[:, :, Ci:]) != 0
        if bad.any():
            b, t, c = _first(bad)
            problems.append(f"tap {j0}: channel {Ci + c} >= Ci not +0 at utterance {b} row {t} (row {t % tile} of tile {t // tile})")
        y = y[:, :, :Ci]
        r = torch.arange(y.shape[1], device=dev) * stride + j0 * dil - pad
        ok = (r >= 0) & (r < T)
        bad = _bits(y[:, ~ok]) != 0
        if bad.any():
            b, i, c = _first(bad)
            t = int((~ok).nonzero()[i])
            problems.append(f"tap {j0}: zero padding not +0 at utterance {b} output row {t} (row {t % tile} of tile "
                            f"{t // tile}) channel {c}")
        rows, vals = r[ok], y[:, ok]
        seen = filled[rows]
        if seen.any():
            bad = _bits(vals[:, seen]) != _bits(S[:, rows[seen]])
            if bad.any():
                b, i, c = _first(bad)
                t = int(ok.nonzero()[seen.nonzero()[i]])
                problems.append(f"tap {j0}: staged row {int(rows[seen][i])} read at output row {t} (row {t % tile} of "
                                f"tile {t // tile}) channel {c} utterance {b} differs from an earlier tap's read")
        S[:, rows[~seen]] = vals[:, ~seen]
        filled[rows] = True
    if not bool(filled.all()):
        problems.append(f"staged rows never read: {filled.logical_not().nonzero().flatten().tolist()[:8]}")
    return S, problems


def polyphase_expect(S, j0, *, ups, ups_pad, refl):
    """the polyphase ConvTranspose's exact output for delta_weights_T(.., j0) on staged rows S [B, T, C]: row q lands at
    t = q ups + j0 - ups_pad when that is in [0, T ups), shifted by refl, and row 0 mirrors row 2 (ReflectionPad(1, 0));
    every other row is +0 -> [B, T ups + refl, C]"""
    B, T, Cc = S.shape
    E = torch.zeros(B, T * ups + refl, Cc, dtype=S.dtype, device=S.device)
    t = torch.arange(T, device=S.device) * ups + j0 - ups_pad
    ok = (t >= 0) & (t < T * ups)
    E[:, t[ok] + refl] = S[:, ok]
    if refl:
        E[:, 0] = E[:, 2]
    return E


def probe_readout_T(run, *, T, Ci, Co, ups, ups_pad, refl):
    """probe_readout for the polyphase ConvTranspose (k = 2 ups): run(j0, m) uses delta_weights_T(Ci, Co, 2 ups, j0, m)
    and returns y [B, T ups + refl, Co].  S is read through tap j0 = ups_pad (row q at t = q ups, every q in range);
    every tap's whole output must then equal polyphase_expect(S, j0) bit for bit -> (S [B, T, Ci], problems)."""
    nb = (Ci + Co - 1) // Co
    ys = {j0: torch.cat([run(j0, m) for m in range(nb)], -1) for j0 in range(2 * ups)}
    S = ys[ups_pad][:, refl:T * ups + refl:ups, :Ci].contiguous()
    problems = []
    for j0, y in ys.items():
        E = polyphase_expect(S, j0, ups=ups, ups_pad=ups_pad, refl=refl)
        bad = _bits(y[:, :, :Ci]) != _bits(E)
        if bad.any():
            b, t, c = _first(bad)
            problems.append(f"tap {j0} (phase {j0 % ups}): utterance {b} output row {t} channel {c} is "
                            f"{float(y[b, t, c])}, expected {float(E[b, t, c])}")
        if bool((_bits(y[:, :, Ci:]) != 0).any()):
            problems.append(f"tap {j0}: channels >= Ci not +0")
    return S, problems


# ---- waveform back end and integer path (tests/test_gpu_backend.py, test_refops_backend.py) ----
# Plain parameters throughout (no Spec: Spec.check() admits the shipped geometry only).  numpy, fp64 unless stated.

def phase_prefix_ref(f0, nh, hop, sr):
    """f0 [B, T80] fp32 -> the per-80-fps-frame phase prefix [B, nh, T80] fp64, wrapped every frame: the recurrence of
    oracle.frame_phase_prefix (acc = frac(acc + hop * (f0 (h + 1) / sr)), one IEEE fp64 rounding per operation)."""
    f = np.asarray(f0, np.float32).astype(np.float64)
    B, T = f.shape
    inc = f[:, None, :] * np.arange(1, nh + 1, dtype=np.float64)[None, :, None] / np.float64(sr)
    out = np.zeros((B, nh, T))
    acc = np.zeros((B, nh))
    for k in range(T):
        out[:, :, k] = acc
        acc = acc + np.float64(hop) * inc[:, :, k]
        acc = acc - np.floor(acc)
    return out


def source_theta32(f0, seeds, *, hop, nh, sr, first_phase_zero=True, n=None):
    """the wrapped phase theta [B, nh, len(n)] fp32 (cycles) at the samples n (None: all N = T80 hop) with the fp32 operation sequence of oracle.harmonic_source:
    fadd(prefix32, ph0), fadd(., fmul(j, finc)), t - floor(t), finc = fdiv(fmul(f0, h + 1), sr) -- one rounding each, no
    contraction.  The fundamental starts at phase 0 (first_phase_zero; False is a defect the self-checks plant).
    -> (theta, prefix32 [B, nh, T80], keys [B][nh])"""
    from oracle.stzs_ref import initial_phase, stream_key
    f = np.asarray(f0, np.float32)
    B, T = f.shape
    n = np.arange(T * hop) if n is None else np.asarray(n)
    k = n // hop
    j = (n - k * hop + 1).astype(np.float32)
    pre = phase_prefix_ref(f, nh, hop, sr).astype(np.float32)
    theta = np.zeros((B, nh, len(n)), np.float32)
    keys = []
    for b in range(B):
        keys.append([stream_key(int(seeds[b]), h) for h in range(nh)])
        for h in range(nh):
            ph0 = np.float32(0.0) if h == 0 and first_phase_zero else initial_phase(keys[b][h])
            finc = (f[b] * np.float32(h + 1)).astype(np.float32) / np.float32(sr)
            t = (pre[b, h] + ph0).astype(np.float32)[k]
            t = (t + (j * finc[k]).astype(np.float32)).astype(np.float32)
            theta[b, h] = (t - np.floor(t)).astype(np.float32)
    return theta, pre, keys


def _mix32(x):
    """lowbias32 on 32-bit values carried in uint64 lanes (the counter RNG's hash, restated)"""
    m = np.uint64(0xFFFFFFFF)
    x = np.asarray(x, dtype=np.uint64) & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def uniforms24(key, idx):
    """the two 24-bit uniforms of counter_normal(key, idx): u1 in (0, 1], u2 in [0, 1), exact in fp32 and fp64"""
    i = np.asarray(idx, dtype=np.uint64)
    a = _mix32(np.uint64(key) ^ _mix32(i * np.uint64(2)))
    b = _mix32(np.uint64(key) ^ _mix32(i * np.uint64(2) + np.uint64(1)))
    return ((a >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0, (b >> np.uint64(8)).astype(np.float64) / 16777216.0


def reflect_index(p, N, n_fft):
    """padded sample index p (centre=True) -> signal index, torch's reflect padding: -n on the left, 2 (N - 1) - n on
    the right"""
    n = np.asarray(p) - n_fft // 2
    n = np.where(n < 0, -n, n)
    return np.where(n >= N, 2 * (N - 1) - n, n)


def source_ref(f0, seeds, merge_w, *, hop, n_fft, hop_s, nh, sr, sine_amp, noise_std, voiced_thr, frames=None):
    """the harmonic source and its STFT.  f0 [B, T80] fp32, seeds [B], merge_w [nh + 1] fp32 (weights, bias).  theta is
    source_theta32 (the part the kernel shares bit for bit); everything after it is fp64: sine, Box-Muller on the same
    24-bit uniforms, merge, tanh, reflect padding, periodic Hann, DFT.  frames: the frame indices to transform (None =
    all Tf = N / hop_s + 1) -> dict(bins [B, len(frames), 2 nb] (real | imag), A1 = sum_i win_i, A2 [B, len(frames)] =
    sum_i |x_i win_i|, x [B, N] (NaN at the samples no chosen frame reads), prefix32 [B, nh, T80])."""
    f = np.asarray(f0, np.float32)
    w = np.asarray(merge_w, np.float32).astype(np.float64)
    B, T = f.shape
    N = T * hop
    Tf = N // hop_s + 1
    fr = np.arange(Tf) if frames is None else np.asarray(frames)
    i = np.arange(n_fft)
    src = reflect_index(fr[:, None] * hop_s + i[None, :], N, n_fft)  # [F, n_fft] signal indices
    n = np.unique(src)
    theta, pre, keys = source_theta32(f, seeds, hop=hop, nh=nh, sr=sr, n=n)
    voiced = (f > np.float32(voiced_thr))[:, n // hop]
    namp = np.where(voiced, np.float64(np.float32(noise_std)), np.float64(np.float32(sine_amp)) / 3.0)
    x = np.full((B, N), np.nan)
    for b in range(B):
        acc = np.zeros(len(n))
        for h in range(nh):
            u1, u2 = uniforms24(keys[b][h], n)
            z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)
            sine = np.float64(np.float32(sine_amp)) * np.sin(2.0 * math.pi * theta[b, h].astype(np.float64))
            acc = acc + w[h] * (sine * voiced[b] + namp[b] * z)
        x[b, n] = np.tanh(acc + w[nh])
    win = 0.5 - 0.5 * np.cos(2.0 * math.pi * i / n_fft)
    xi = x[:, src] * win  # [B, F, n_fft]
    nb = n_fft // 2 + 1
    ang = 2.0 * math.pi * np.outer(i, np.arange(nb)) / n_fft
    bins = np.concatenate([xi @ np.cos(ang), -(xi @ np.sin(ang))], -1)
    return dict(bins=bins, A1=float(win.sum()), A2=np.abs(xi).sum(-1), x=x, prefix32=pre)


def istft_ref(post, n_fft, hop_s):
    """post [B, Tf, >= 2 nb] fp32 (log-magnitudes | phase arguments) -> (wav [B, (Tf - 1) hop_s], S the same shape, min
    env), fp64 from the fp32 inputs: mag = exp(m), ph = sin(p), irfft by the explicit DFT (the imaginary parts of DC
    and Nyquist do not enter), periodic Hann, overlap-add, window-square envelope, centre trim.  S = sum over a
    sample's frames and bins of |mag_k| c_k win_i / (n_fft env), c_k = 1 for DC and Nyquist and 2 otherwise: the
    magnitude its rounding errors scale with.  min env is taken over the emitted samples."""
    p = np.asarray(post, np.float32).astype(np.float64)
    B, Tf = p.shape[:2]
    nb = n_fft // 2 + 1
    mag, ph = np.exp(p[:, :, :nb]), np.sin(p[:, :, nb:2 * nb])
    re, im = mag * np.cos(ph), mag * np.sin(ph)
    i = np.arange(n_fft)
    ang = 2.0 * math.pi * np.outer(np.arange(nb), i) / n_fft
    c = np.full(nb, 2.0)
    c[0] = c[-1] = 1.0
    win = 0.5 - 0.5 * np.cos(2.0 * math.pi * i / n_fft)
    fr = ((re * c) @ np.cos(ang) - (im * c) @ np.sin(ang)) / n_fft * win  # [B, Tf, n_fft]
    fs = ((mag * c).sum(-1, keepdims=True) / n_fft) * win                   # the same sum on magnitudes
    M = (Tf - 1) * hop_s + n_fft
    y, s, env = np.zeros((B, M)), np.zeros((B, M)), np.zeros(M)
    for t in range(n_fft):
        sl = slice(t, t + Tf * hop_s, hop_s)
        y[:, sl] += fr[:, :, t]
        s[:, sl] += fs[:, :, t]
        env[sl] += win[t] ** 2
    keep = slice(n_fft // 2, n_fft // 2 + (Tf - 1) * hop_s)
    env = env[keep]
    return y[:, keep] / env, s[:, keep] / env, float(env.min())


def istft_halo(n_fft, hop_s):
    """frames before a chunk that still reach its samples: ceil(n_fft / hop_s) - 1"""
    return -(-n_fft // hop_s) - 1


def istft_span_ref(f0, Fc, final, n_fft, hop_s):
    """the output samples [n0, n1) a streaming chunk of frames [f0, f0 + Fc) emits, from include/stzs.h's wording:
    every sample whose overlapping frames are all known -- padded sample m (output n = m - n_fft / 2) overlaps frames
    up to m // hop_s, so m < (f0 + Fc) hop_s -- that no earlier chunk has emitted; the final chunk emits everything up
    to (f0 + Fc - 1) hop_s -> (n0, n1, halo)"""
    n0 = max(0, f0 * hop_s - n_fft // 2)
    n1 = (f0 + Fc - 1) * hop_s if final else (f0 + Fc) * hop_s - n_fft // 2
    return n0, max(n0, n1), istft_halo(n_fft, hop_s)


def durations_ref(logits):
    """logits [B, T, nbins] fp32 -> (dur int32 = max(1, round-half-even(sum)), sum fp64 of the sigmoids, the distance of
    the sum from the nearest half-integer): the duration head in fp64"""
    s = (1.0 / (1.0 + np.exp(-np.asarray(logits, np.float32).astype(np.float64)))).sum(-1)
    return np.maximum(np.rint(s), 1).astype(np.int32), s, np.abs(s - np.floor(s) - 0.5)


def align_ref(dur, T40):
    """dur [B, T] int32 (zeros anywhere) -> (idx [B, T40] int32: the token that owns aligned frame f, -1 from the row's
    own total on; total [B] int32)"""
    d = np.asarray(dur)
    idx = np.full((d.shape[0], T40), -1, np.int32)
    for b in range(d.shape[0]):
        own = np.repeat(np.arange(d.shape[1], dtype=np.int32), d[b])[:T40]
        idx[b, :len(own)] = own
    return idx, d.sum(1).astype(np.int32)


E_SIN, E_BM, E_T = 1e-6, 2e-6, 3e-6  # the accuracy claims of csrc/source.hip (sine, Box-Muller) and csrc/istft.hip
E_RR = 2.0 ** -22                    # the iSTFT's range reduction of a phase argument beyond pi (istft_bound)


def source_bound(ref, merge_w, *, n_fft, sine_amp, noise_std):
    """the per-element bound on fp32 bins against source_ref's dict: d A1 + (n_fft + 4) 2^-24 A2, d = sum_h |mw_h|
    (sine_amp E_SIN + namp_max E_BM) + 4 2^-24 the per-sample allowance (tanh's slope is at most 1; four roundings of
    values below 1 in the merge and the tanh), then n_fft accumulation steps of the windowed DFT -> [B, F, 1]"""
    w = np.abs(np.asarray(merge_w, np.float64)[:-1]).sum()
    d = w * (sine_amp * E_SIN + max(noise_std, sine_amp / 3.0) * E_BM) + 4 * 2.0 ** -24
    return (d * ref["A1"] + (n_fft + 4) * 2.0 ** -24 * ref["A2"])[..., None]


def istft_bound(S, n_fft, hop_s, reduced):
    """the per-sample bound against istft_ref's S: (E_T + (nb + halo + 6) 2^-24) S -- three chained hardware
    transcendentals, nb accumulation steps of the DFT, halo + 1 of the overlap-add, the window, the envelope and the
    division.  reduced (the large-argument class, |p| up to 2^17): the two-constant reduction xr = fma(-k, lo,
    fma(-k, hi, p)) rounds twice at |xr| < 4 (half an ulp of 2^-22 each): |d xr| <= 2^-22 = E_RR, which sin, cos and
    the magnitude carry into the sample with slope at most 1, i.e. as E_RR S."""
    nb = n_fft // 2 + 1
    return (E_T + (E_RR if reduced else 0.0) + (nb + istft_halo(n_fft, hop_s) + 6) * 2.0 ** -24) * S


def f0_case(B, T80, thr, key):
    """F0 [B, T80] fp32 for a source case: voiced 80..400 Hz with, where the row is long enough, a stretch of exact
    zeros, one frame exactly at thr (unvoiced), one at nextafter(thr, inf) (voiced) and one at 900 Hz; shorter rows
    take these values in turn.  Even rows start and end voiced, odd rows unvoiced (a one-row case by its key)."""
    g = np.random.default_rng(zlib_key(key))
    f = g.uniform(80.0, 400.0, (B, T80)).astype(np.float32)
    special = [np.float32(0.0), np.float32(thr), np.nextafter(np.float32(thr), np.float32(np.inf)), np.float32(900.0)]
    for b in range(B):
        if T80 >= 13:
            f[b, 3:6] = 0.0
            f[b, 7], f[b, 8], f[b, 9] = special[1], special[2], special[3]
            if T80 > 40:
                f[b, T80 // 2:T80 // 2 + 5] = 0.0
        else:
            for k in range(T80):
                f[b, k] = special[(b + k + zlib_key(key)) % 4]
        if (b + (zlib_key(key) if B == 1 else 0)) % 2 and T80 >= 13:
            f[b, 0] = f[b, -1] = 0.0
    return f


def zlib_key(key):
    import zlib
    return zlib.crc32(repr(key).encode())


def post_case(B, Tf, n_fft, cls, key, ldp=None):
    """conv_post rows [B, Tf, ldp] fp32 for an iSTFT case, NaN beyond the 2 nb used columns: log-magnitudes N(0, 0.5)
    with one bin at +10 and one at -100 per utterance, phase arguments of class "small" N(0, 2), "mid" N(0, 600) or
    "large" uniform in +-(2^17 - 1) with two values within 1 of +-2^17"""
    nb = n_fft // 2 + 1
    ldp = n_fft + 6 if ldp is None else ldp
    g = np.random.default_rng(zlib_key(("post",) + tuple(key)))
    p = np.full((B, Tf, ldp), np.nan, np.float32)
    p[:, :, :nb] = g.normal(0.0, 0.5, (B, Tf, nb))
    if cls == "small":
        p[:, :, nb:2 * nb] = g.normal(0.0, 2.0, (B, Tf, nb))
    elif cls == "mid":
        p[:, :, nb:2 * nb] = g.normal(0.0, 600.0, (B, Tf, nb))
    else:
        assert cls == "large", cls
        lim = 2.0 ** 17 - 1
        p[:, :, nb:2 * nb] = g.uniform(-lim, lim, (B, Tf, nb))
        p[0, Tf // 2, nb + 1] = np.float32(2.0 ** 17 - 0.5)
        p[B - 1, Tf - 1, 2 * nb - 1] = np.float32(-(2.0 ** 17) + 0.25)
    for b in range(B):
        p[b, (b + 1) % Tf, (3 + b) % nb] = 10.0
        p[b, (Tf - 1 - b) % Tf, (5 + b) % nb] = -100.0
    return p


# ---- the cases tests/test_gpu_backend.py runs, shared with the CPU self-checks ----
SHIPPED = dict(hop=300, n_fft=20, hop_s=5, sr=24000.0, sine_amp=0.1, noise_std=0.003, voiced_thr=10.0)
# the iSTFT geometries of the GPU file, (n_fft, hop_s) -> halo
ISTFT_GEOMS = {(20, 5): 3, (20, 4): 4, (20, 10): 1, (20, 3): 6, (20, 2): 9, (16, 4): 3, (16, 8): 1, (16, 2): 7}
# the GPU file's duration shapes and the seed of each (chosen so that the reference alone keeps the tie share < 1 %)
DUR_NBINS, DUR_ROWS = (1, 7, 8, 9, 50), (1, 255, 256, 257)


def merge_weights(nh, key=0):
    g = np.random.default_rng(1000 + nh + key)
    return (g.normal(0.0, 0.3, nh + 1)).astype(np.float32)


def dur_logits(rows, nbins, seed=0):
    """[1, rows, nbins] fp32 logits whose sigmoid sums spread over [0, nbins]"""
    g = np.random.default_rng(77 + 1000 * nbins + rows + seed)
    return (g.normal(0.0, 2.0, (1, rows, nbins)) + g.normal(0.0, 1.5, (1, rows, 1))).astype(np.float32)


def dur_tie_width(nbins):
    """an fp32 serial sum of nbins sigmoids is within nbins * 2^-23 * nbins of the fp64 sum"""
    return nbins * 2.0 ** -23 * nbins


# ---- LSTM recurrence: the teacher-forced fp64 reference (tests/test_gpu_lstm_parity.py, test_refops_lstm.py) ----
# A free-running bf16 recurrence amplifies every rounding flip of h over the remaining steps, so a per-element bound on
# it is useless.  Teacher forcing removes the amplification: at every step the reference takes as h_{t-1} the values the
# kernel itself stored in y at the previous position of that direction (zeros at the first step) -- in bf16 mode
# bit for bit what the workgroups exchanged -- and carries only the cell state c, in fp64, with a running error bound.

U32 = 2.0 ** -24  # the unit roundoff of fp32


def split_hi_lo(y):
    """fp32 -> (hi, lo) fp64 as the precise kernel splits the h it exchanges: hi = bf16(y) to nearest even, lo =
    bf16(y - hi) (the difference is exact in fp32)"""
    y = y.float()
    hi = y.to(torch.bfloat16).float()
    return hi.double(), (y - hi).to(torch.bfloat16).double()


def half_ulp_bf16(h):
    """half the spacing of bf16 at round_bf16(h) (exact, not 2^-8 |h|, which is up to twice as loose); 0 at h == 0"""
    r = round_bf16(torch.where(h == 0, torch.ones_like(h), h)).double()
    _, e = torch.frexp(r)  # |r| = m 2^e, m in [0.5, 1): the spacing above |r| is 2^(e - 8)
    return torch.where(h == 0, torch.zeros_like(h), torch.ldexp(torch.ones_like(h), e.clamp_min(-125) - 9))


def _sig_err(pre, e_pre):
    # sigmoid = rcp(1 + exp(-x)), exp(x) = v_exp_f32(x log2 e): the argument product's rounding |x| u relative, v_exp
    # and v_rcp 1 ulp each, the add 1/2 ulp; doubled as dense_ratio doubles its total; sigmoid' <= 1/4, sigmoid <= 1
    return e_pre / 4 + (pre.abs() + 3) * 2 * U32


def _tanh_err(pre, e_pre=0.0):
    # tanh = 1 - 2 rcp(1 + exp(2x)) with one fma: twice the argument, 1 + 1 + 1/2 + 1/2 ulp, doubled; tanh' <= 1
    return e_pre + (2 * pre.abs() + 3) * 4 * U32


def lstm_tf_ref(gx, w_hh, y, H, ndir, lens=None, precise=False):
    """The teacher-forced reference of stzs_lstm.  gx [B, T, ndir 4H] fp32 (gate order i, f, g, o per direction: the C
    ABI's layout), w_hh a list of ndir [4H, H] tensors as the kernel holds them (bf16 mode: the bf16-rounded values;
    precise: the (hi, lo) pair of stzs.weights.split_bf16), y [B, T, ndir H] what the kernel stored (bf16 | fp32), lens
    [B] | None -> (h_ref, E_h) fp64 [B, T, ndir H]: the output given the kernel's own h_{t-1}, and the bound of what an
    fp32 evaluation may differ from it by.

    Per step and gate, bf16 mode: pre = gx + h_prev W^T, terms = |gx| + |h_prev| |W|^T, e_pre = 2 (H + 4) 2^-24 terms
    (dense_ratio's constants).  Precise: h_prev = hi + lo as split_hi_lo, pre = gx + h_lo W_hi + h_hi W_lo + h_hi W_hi
    (the kernel's three products; lo lo is absent on purpose), terms the same on absolute values, e_pre = 2 (3H + 4)
    2^-24 terms.  Gate errors (u = 2^-24): sigmoid e = e_pre / 4 + (|pre| + 3) 2u, tanh e = e_pre + (2 |pre| + 3) 4u
    (_sig_err / _tanh_err: hardware v_exp_f32 and v_rcp_f32 at 1 ulp each).  The same forms serve the precise mode's
    libm expf / tanhf, which rests on the device library being within about 5 fp32 ulps there -- unconfirmed: its
    accuracy table was not at hand when this was written.
    Cell: c = f c + i g,
    E_c <- f E_c + |c_prev| e_f + e_f E_c + |g| e_i + i e_g + e_i e_g + 2u (|f c_prev| + |i g|);
    output: h = o tanh(c), E_h = |tanh c| e_o + (o + e_o) (E_c + A_tanh(c)) + u |h|, A_tanh = _tanh_err(c).
    Ragged rows: where t >= clamp(lens[b], 1, T), c, E_c, h and E_h are 0, as the kernel sets them after its update."""
    B, T = gx.shape[:2]
    assert gx.shape[2] == ndir * 4 * H and y.shape == (B, T, ndir * H) and len(w_hh) == ndir
    gx, yd = gx.double(), y.double()
    K = 3 * H if precise else H
    ln = None if lens is None else torch.as_tensor(lens).long().clamp(1, T)
    h_ref, E_h = torch.zeros(B, T, ndir * H, dtype=torch.float64), torch.zeros(B, T, ndir * H, dtype=torch.float64)
    for d in range(ndir):
        if precise:
            whi, wlo = (w.double().t() for w in w_hh[d])
        else:
            w = w_hh[d].double().t()
        c = torch.zeros(B, H, dtype=torch.float64)
        Ec = torch.zeros(B, H, dtype=torch.float64)
        for s in range(T):
            t = s if d == 0 else T - 1 - s
            tp = t - 1 if d == 0 else t + 1
            g_t = gx[:, t, d * 4 * H:(d + 1) * 4 * H]
            hp = yd[:, tp, d * H:(d + 1) * H] if s else torch.zeros(B, H, dtype=torch.float64)
            if precise:
                hi, lo = split_hi_lo(y[:, tp, d * H:(d + 1) * H]) if s else (hp, hp)
                pre = g_t + lo @ whi + hi @ wlo + hi @ whi
                terms = g_t.abs() + lo.abs() @ whi.abs() + hi.abs() @ wlo.abs() + hi.abs() @ whi.abs()
            else:
                pre = g_t + hp @ w
                terms = g_t.abs() + hp.abs() @ w.abs()
            e_pre = 2.0 * (K + 4) * U32 * terms
            pi, pf, pg, po = pre.split(H, 1)
            ei, ef, eg, eo = (_sig_err(p, e) if k != 2 else _tanh_err(p, e)
                              for k, (p, e) in enumerate(zip((pi, pf, pg, po), e_pre.split(H, 1))))
            ig, fg, gg, og = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
            Ec = (fg * Ec + c.abs() * ef + ef * Ec + gg.abs() * ei + ig * eg + ei * eg
                  + 2 * U32 * ((fg * c).abs() + (ig * gg).abs()))
            c = fg * c + ig * gg
            th = torch.tanh(c)
            h = og * th
            Eh = th.abs() * eo + (og + eo) * (Ec + _tanh_err(c)) + U32 * h.abs()
            if ln is not None:
                keep = (t < ln)[:, None].double()
                c, Ec, h, Eh = c * keep, Ec * keep, h * keep, Eh * keep
            h_ref[:, t, d * H:(d + 1) * H], E_h[:, t, d * H:(d + 1) * H] = h, Eh
    return h_ref, E_h


def lstm_tf_check(y, h_ref, E_h, bf16_out):
    """y against lstm_tf_ref's (h_ref, E_h) -> (ratio, flip_share).  ratio = max |y - h_ref| / bound with bound =
    half_ulp_bf16(h_ref) + E_h (1 + 2^-8) for a bf16 output (the rounding of a value within E_h of h_ref) and bound = E_h
    for an fp32 one; where the bound is 0 (a ragged row's tail) anything but an exact 0 gives inf.  flip_share (bf16
    output; 0.0 otherwise): the share of the non-zero reference elements whose bits differ from round_bf16(h_ref).
    The first must be <= 1, the second <= 0.01 (staged_check's cap)."""
    d = (y.double() - h_ref).abs()
    bound = half_ulp_bf16(h_ref) + E_h * (1 + 2.0 ** -8) if bf16_out else E_h
    ratio = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d == 0, 0.0, float("inf")).double())
    share = 0.0
    if bf16_out:
        nz = h_ref != 0
        want = round_bf16(torch.where(nz, h_ref, torch.ones_like(h_ref)))
        diff = (_bits(y.to(torch.bfloat16)) != _bits(want)) & nz
        share = diff.sum().item() / max(int(nz.sum().item()), 1)
    return ratio.max().item(), share


def lstm_emulate(gx, w_hh, H, ndir, lens=None, mutate=None, precise=False):
    """An fp32 model of the kernel on the CPU: h exchanged as bf16 (precise: as the hi | lo pair, y fp32), c in fp32,
    torch's sigmoid / tanh.  Arguments as lstm_tf_ref -> y [B, T, ndir H] bf16 (precise: fp32).  mutate: one mistake
    for tests/test_refops_lstm.py -- "w" one W_hh element off by 0.05, "swap_if" the i and f blocks of the recurrent
    product swapped, "stale" h_{t-2} used from step 2 on, "zero_row" the longest row's exchanged h zeroed at one step per
    direction with its y correct, "c_drift" c scaled by 1 + 1e-4 every step."""
    B, T = gx.shape[:2]
    ln = None if lens is None else torch.as_tensor(lens).long().clamp(1, T)
    y = torch.zeros(B, T, ndir * H, dtype=torch.float32 if precise else torch.bfloat16)
    zrow = 0 if ln is None else int(ln.argmax())  # "zero_row": the longest row
    zlen = T if ln is None else int(ln[zrow])
    for d in range(ndir):
        ws =[w.float().clone() for w in w_hh[d]] if precise else [w_hh[d].float().clone()]
        if mutate == "w":
            ws[0][2 * H + 5, 3] += 0.05
        c = torch.zeros(B, H)
        sent = [torch.zeros(B, H)]  # what was exchanged, per step (fp32 values of the bf16 | hi + lo)
        for s in range(T):
            t = s if d == 0 else T - 1 - s
            hp = sent[-2] if mutate == "stale" and s >= 2 else sent[-1]
            if precise:
                hi = hp.to(torch.bfloat16).float()
                lo = (hp - hi).to(torch.bfloat16).float()
                rec = lo @ ws[0].t() + hi @ ws[1].t() + hi @ ws[0].t()
            else:
                rec = hp @ ws[0].t()
            if mutate == "swap_if":
                rec = torch.cat([rec[:, H:2 * H], rec[:, :H], rec[:, 2 * H:]], 1)
            pi, pf, pg, po = (gx[:, t, d * 4 * H:(d + 1) * 4 * H].float() + rec).split(H, 1)
            c = torch.sigmoid(pf) * c + torch.sigmoid(pi) * torch.tanh(pg)
            if mutate == "c_drift":
                c = c * (1 + 1e-4)
            h = torch.sigmoid(po) * torch.tanh(c)
            if ln is not None:
                keep = (t < ln)[:, None]
                c, h = c * keep, h * keep
            h = h if precise else h.to(torch.bfloat16)
            y[:, t, d * H:(d + 1) * H] = h
            x = h.float().clone()
            if mutate == "zero_row" and t == (0 if d == 0 else zlen - 1):  # (a step whose h the next one reads)
                x[zrow] = 0
            sent.append(x)
    return y


# ---- the linears: exact operand probes and per-element bounds (tests/test_gpu_linear_probe.py, test_refops_linear.py,
# the --linear-cases mode of tools/dispatch_trace.py) ----
# A linear is a conv with one tap: with delta_weights(Co, Ci, 1, 0, m), bias 0 and no epilogue operands the output IS
# the kernel's staged A operand, through split-K, the wave-partial sums and the fp8 dequantisation (every partial is
# 0 + x).

from collections import namedtuple

LIN_DT = {"bf16": torch.bfloat16, "f32": torch.float32, "f8": torch.float8_e4m3fn}
LIN_POISON = 2.0 ** 100   # finite: 0 * poison = 0
LIN_POISON_F8 = 0x7E      # e4m3fn 448, the largest finite code
LIN_SENT = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FC0A5A5}  # NaN payloads: a write of any value shows
LIN_ROWS = ((1, 1), (3, 5), (1, 64), (5, 13), (2, 50), (3, 43))  # (B, T): 1, 15, 64, 65, 100, 129 rows

# kern: glds (gemm_glds, 64-row tiles) | glds128 (its 128-row tile) | f8 (gemm_glds fp8) | rows (gemm_rows) | rows16;
# Z: K slices (0: unsplit); idt / odt: keys of LIN_DT; ypads: guarded()'s pads of y; ids: STZS_CONV_LINEAR_IDS;
# cscale: the fp32 input's scale
LinCase = namedtuple("LinCase", "kern B T Ci Co Z idt odt ypads ids cscale", defaults=("bf16", "bf16", (2, 8, 8), 0, 1.0))


def lin_id(c):
    return (f"{c.kern}-{c.B}x{c.T}-{c.Ci}to{c.Co}-Z{c.Z}-{c.idt}-{c.odt}" + ("-ldy24" if c.ypads[1:] == (0, 0) else "") +
            ("-ids" if c.ids else "") + (f"-cs{c.cscale}" if c.cscale != 1.0 else ""))


def lin_ci_pad(c):
    """stzs.weights.pack_conv's / pack_conv_f8's K padding, restated"""
    if c.kern == "f8":
        return (c.Ci + 63) // 64 * 64
    cic = 32 if c.Ci <= 32 else (64 if c.Ci <= 64 else 128)
    return (c.Ci + cic - 1) // cic * cic


def gemm_tile_rows(M, co_pad, ncu):
    """csrc/gemm.hip gemm_launch's tile height, restated: 128-row tiles run two workgroups per CU, 64-row tiles three,
    and a 64-row tile costs 0.6 of a 128-row one -- 64 where 6 r64 < 10 r128 (r: rounds of resident workgroups)"""
    gy = co_pad // 128
    n128, n64 = (M + 127) // 128 * gy, (M + 63) // 64 * gy
    r128, r64 = (n128 + 2 * ncu - 1) // (2 * ncu), (n64 + 3 * ncu - 1) // (3 * ncu)
    return 64 if 6 * r64 < 10 * r128 else 128


def gemm_tile128_rows(ncu, Co=2048, T=50, limit=12800):
    """the row count of the 128-row-tile probe: 64 x 50 rows where the rule gives them the 128-row tile (256 CUs),
    else the smallest multiple of T up to `limit` that it does; None if there is none"""
    for M in [64 * T] + list(range(T, limit + 1, T)):
        if gemm_tile_rows(M, (Co + 127) // 128 * 128, ncu) == 128:
            return M
    return None


def linear_cases(ncu=256):
    """the identity-probe table of tests/test_gpu_linear_probe.py (section A): axis sweeps over the K-step counts, the
    row counts, the output widths and the dtypes of every kernel form, not their product"""
    C, out = LinCase, []
    big = (3, 43)
    # gemm_glds, 64-row tiles: K-steps 1, 2, 4, 12, 16; Ci < ci_pad (22, 80); rows; widths; the scalar epilogue
    out += [C("glds", *big, Ci, 200, 0, "bf16", o) for Ci in (22, 64, 80, 384, 512) for o in ("bf16", "f32")]
    out += [C("glds", B, T, 80, 80, 0) for B, T in LIN_ROWS if (B, T) != big]
    out += [C("glds", 5, 13, 128, Co, 0, "bf16", "f32") for Co in (8, 80, 128, 384)] + [C("glds", 5, 13, 128, 8, 0)]
    out += [C("glds", *big, 64, 22, 0, "bf16", o, (2, 0, 0)) for o in ("bf16", "f32")]
    M = gemm_tile128_rows(ncu)
    if M is not None:
        out += [C("glds128", M // 50, 50, 32, 2048, 0, "bf16", o) for o in ("bf16", "f32")]
        if gemm_tile_rows(3137, 2048, ncu) == 128:
            out += [C("glds128", 1, 3137, 32, 2048, 0)]
        if gemm_tile_rows(3073, 2048, ncu) == 128:
            out += [C("glds128", 7, 439, 32, 2048, 0)]  # (one row in the last 128-row tile)
    # split-K: slices of 1, 2, 3 and 6 K-steps
    for Ci, Z in ((64, 2), (128, 2), (128, 4), (384, 4), (384, 2)):
        out += [C("glds", *big, Ci, 200, Z, "bf16", o, ids=i) for o in ("bf16", "f32") for i in (0, 1)]
    out += [C("glds", B, T, 128, 80, 4, "bf16", "f32") for B, T in ((1, 1), (5, 13))]
    out += [C("glds", *big, 128, 22, 2, "bf16", "f32", (2, 0, 0))]
    # fp8: K-steps 1, 2, 3, 5
    out += [C("f8", *big, Ci, 200, 0, "f8", o) for Ci in (64, 128, 192, 320) for o in ("f32", "bf16")]
    out += [C("f8", B, T, 128, 80, 0, "f8", "f32") for B, T in LIN_ROWS[:4]]
    out += [C("f8", *big, 64, 22, 0, "f8", "f32", (2, 0, 0))]
    # gemm_rows: Z x K-steps per wave 1, 2, 4, 16; rows across the 64 / 128-row block switch; widths; dtypes
    for kern, KZ in (("rows", ((128, 0), (256, 0), (256, 2), (512, 0), (512, 2), (512, 4), (2048, 0))),
                     ("rows16", ((128, 0), (256, 0), (512, 0), (1024, 0), (2048, 0), (256, 2), (1024, 2), (512, 4),
                                 (2048, 4)))):
        out += [C(kern, *big, Ci, 200, Z, "bf16", "f32") for Ci, Z in KZ]
        out += [C(kern, *big, 256, 80, Z, "bf16", "bf16") for Z in (0, 2)]
        out += [C(kern, B, T, 256, 80, 2) for B, T in LIN_ROWS if (B, T) != big]
        out += [C(kern, B, T, 128, 80, 0, "bf16", "f32") for B, T in LIN_ROWS if (B, T) != big]
        out += [C(kern, 5, 13, 128, Co, 0, "bf16", "f32") for Co in (16, 22, 200)]
        out += [C(kern, 5, 13, 256, 22, 2, "bf16", "f32", (2, 0, 0))]
        out += [C(kern, 5, 13, 256, 80, Z, "f32", "f32", cscale=0.5) for Z in (0, 2)]
    return out


def lin_expected_launch(c):
    """what the case must launch: (a substring of the kernel's name, grid x, y, z) -- the launchers' geometry restated
    (csrc/gemm.hip, rows.hip, lnrows.hip; rows16 unsplit up to 16 K-steps: one 16-column tile per workgroup, the
    default of STZS_ROWS16_WPG)"""
    M, Z = c.B * c.T, max(c.Z, 1)
    if c.kern in ("glds", "glds128", "f8"):
        bt = 128 if c.kern == "glds128" else 64
        return "gemm_glds", (M + bt - 1) // bt, (c.Co + 127) // 128, Z
    if c.kern == "rows":
        blk = 64 if M <= 64 else 128
        return "gemm_rows", (c.Co + 15) // 16, (M + blk - 1) // blk, Z
    wide = Z > 1 or lin_ci_pad(c) // 32 > 16  # (four 16-column tiles per workgroup: the sliced form, and 32 / 64 K-steps)
    return "rows16", (c.Co + 63) // 64 if wide else (c.Co + 15) // 16, (M + 15) // 16, Z


def linear_probe_expect(xs, Co, m=0):
    """the exact output of delta_weights(Co, Ci, 1, 0, m) on the staged operand xs [B, T, Ci]: column co holds
    xs[:, :, co + m Co] where that exists, +0 elsewhere -> [B, T, Co] in xs's dtype"""
    B, T, Ci = xs.shape
    E = torch.zeros(B, T, Co, dtype=xs.dtype, device=xs.device)
    n = max(0, min(Co, Ci - m * Co))
    E[:, :, :n] = xs[:, :, m * Co:m * Co + n]
    return E


def first_diff(got, want):
    """None where got and want agree in bits, else a message naming the first (utterance, row, column)"""
    bad = _bits(got) != _bits(want)
    if not bool(bad.any()):
        return None
    i = _first(bad)
    return (f"{int(bad.sum())} elements differ; first at (utterance, row, column) {i}: got {float(got[i])!r}, "
            f"expected {float(want[i])!r}")


def e4m3_case(B, T, Ci, seed=0):
    """-> (codes uint8 [B, T, Ci], x_scale fp32 [B T]): random finite e4m3fn codes with, in every row that has room,
    both zeros, the smallest and largest subnormals of both signs and +-448; the row scales are powers of two,
    distinct per row (2^(r - R / 2): their products with 448^2 stay normal fp32 / bf16 numbers)"""
    g = torch.Generator().manual_seed(1000 + seed + B * T + Ci)
    codes = torch.randint(0, 256, (B, T, Ci), generator=g, dtype=torch.int32)
    codes = torch.where(codes & 0x7F == 0x7F, codes - 1, codes).to(torch.uint8)  # (0x7F / 0xFF: NaN)
    special = torch.tensor([0x00, 0x80, 0x01, 0x81, 0x07, 0x87, 0x7E, 0xFE], dtype=torch.uint8)
    for r in range(B * T):
        o = (r * 5) % (Ci - 8 + 1)
        codes.view(B * T, Ci)[r, o:o + 8] = special
    R = B * T
    return codes, torch.ldexp(torch.ones(R), torch.arange(R) - R // 2)


def e4m3_value(codes):
    """uint8 codes -> their fp32 values"""
    return codes.view(torch.float8_e4m3fn).float()


def quant_rows_ref(x):
    """stzs_quant_rows restated (include/stzs.h): the power-of-two row scale 2^k, the smallest with amax / 2^k <= 448,
    then RNE e4m3fn codes of x / 2^k -> (codes uint8, scale fp32 [rows])"""
    amax = x.abs().amax(-1)
    m, e = torch.frexp(amax)
    k = torch.where(m <= 0.875, e - 9, e - 8)
    k = torch.where(amax > 0, k, torch.zeros_like(k))
    scale = torch.ldexp(torch.ones_like(amax), k)
    return (x / scale[..., None]).to(torch.float8_e4m3fn).view(torch.uint8), scale


def act_ratio(got, z, terms, K, act, bf16_out):
    """GELU / SiLU epilogue against the fp64 pre-activation z and its terms: the largest |got - act(z)| / bound, bound =
    1.13 (the Lipschitz bound of both) x dense_ratio's accumulation bound + 4e-7 (1 + |z|) (fast_erf 1.5e-7, __expf)
    (+ 2^-8 |ref| for a bf16 output): tests/test_gpu_conv_probe.py test_dense_flat_gemm_act's bound"""
    ref = 0.5 * z * (1 + torch.erf(z / math.sqrt(2))) if act == "gelu" else z / (1 + torch.exp(-z))
    bound = 1.13 * 2 * (K + 4) * 2.0 ** -24 * terms + 4e-7 * (1 + z.abs())
    if bf16_out:
        bound = bound + ref.abs() * 2.0 ** -8
    return ((got.double() - ref).abs() / bound).max().item()


def layernorm_ref64(x, G, Bt, grp, gadd, eps=1e-5):
    """the modulated row LayerNorm in fp64 on the stored rows x [R, C]: (x - mu) rstd (gadd + G[grp]) + Bt[grp]
    -> (ref, terms = (|x| + |mu|) rstd |g| + |Bt|: what its fp32 evaluation errors scale with)"""
    xx = x.double()
    mu, rs = xx.mean(1, keepdim=True), 1 / torch.sqrt(xx.var(1, unbiased=False, keepdim=True) + eps)
    gg = gadd + (G.double()[grp] if G is not None else 0.0)
    bt = Bt.double()[grp] if Bt is not None else torch.zeros_like(xx)
    return (xx - mu) * rs * gg + bt, (xx.abs() + mu.abs()) * rs * abs(gg) + bt.abs()


def layernorm_image_ok(img, ref, terms):
    """tests/test_gpu_norm_edges.py test_row_layernorm_edges' rule for a bf16 image: every element within one bf16 ulp of
    the rounded reference, or within 2^-8 |ref| + 64 2^-24 terms -> (all ok?, largest ulp distance, elements past one)"""
    u = ulp_dist(img, ref.float().to(torch.bfloat16))
    err = (img.double() - ref).abs()
    ok = (u <= 1) | (err <= 2.0 ** -8 * ref.abs() + 64 * 2.0 ** -24 * terms)
    return bool(ok.all()), int(u.max()), int((u > 1).sum())


def lin_x_pads(c, poisoned):
    """guarded()'s pads of a case's x: the columns behind the row reach c0 + ci_pad <= ld (the engine routes a linear
    whose rows are not readable over ci_pad channels away from the GEMMs); fp8 rows are 16-byte aligned"""
    extra = lin_ci_pad(c) - (c.Ci + 7) // 8 * 8
    al = 16 if c.kern == "f8" else 8
    return (3, al, al + extra) if poisoned else (0, 0, extra)


def lin_launch(eng, c, cw, xa, ya, *, x_scale=None, **epi):
    """one linear through the engine's routing: eng.conv(..., collect=[]) fills and routes the stzs_conv_args, the form
    the case names is asserted (flags, splitk, the entry point _conv_entry returns), then the library call is made here.
    (rows16: the engine does not collect a stzs_ln_linear call, so conv() launches it itself, after the same
    assertions.)  -> the args"""
    from stzs import _lib as L
    label, small = lin_id(c), c.kern in ("rows", "rows16")
    rec, entry = [], eng._conv_entry

    def checked(a, *rest, **kw):
        fn, args, fused = entry(a, *rest, **kw)
        if small:
            assert a.flags & L.CONV_ROWS and not a.flags & 8, (label, a.flags)
        else:
            assert a.flags & 8 and not a.flags & L.CONV_ROWS, (label, a.flags)
        want = eng.lib.stzs_ln_linear if c.kern == "rows16" else eng.lib.stzs_conv1d
        assert fn is want and not fused, (label, "entry point")
        assert a.splitk == c.Z if c.Z > 1 else a.splitk <= 1, (label, a.splitk)
        rec.append((a, fn, args))
        return fn, args, fused

    keep = eng.rows16, eng.rows16_maxk
    eng._conv_entry = checked
    eng.rows16, eng.rows16_maxk = c.kern == "rows16", max(eng.rows16_maxk, 2048 if c.kern == "rows16" else 0)
    try:
        eng.conv(cw, xa, ya, collect=None if c.kern == "rows16" else [], rows=max(c.Z, 1) if small else 0,
                 splitk=0 if small else c.Z, cscale=c.cscale, x_scale=x_scale,
                 flags=L.CONV_LINEAR_IDS if c.ids else 0, what=label, **epi)
    finally:
        eng._conv_entry = entry
        eng.rows16, eng.rows16_maxk = keep
    a, fn, args = rec[0]
    if c.kern != "rows16":
        rc = fn(*args, eng.stream())
        assert rc == 0, f"{label}: the library call returned {rc}"
    return a


LIN_PACKED = {}  # packed one-hot weights, by (device, fp8?, Co, Ci, block)


def lin_pack(c, w, b=None, key=None, dev="cpu"):
    """pack (and cache, under `key`) the Linear weight w [Co, Ci] for the case's kernel on `dev`"""
    if key is not None and (dev, key) in LIN_PACKED:
        return LIN_PACKED[dev, key]
    from stzs.weights import Arena, pack_conv, pack_conv_f8
    A = Arena()
    cw = pack_conv_f8(A, "t", w, b) if c.kern == "f8" else pack_conv(A, "t", w, b)
    A.finalize(dev)
    cw.w = A[cw.w]
    cw.b = A[cw.b] if cw.b is not None else None
    if c.kern == "f8":
        cw.wscale = A[cw.wscale]
    cw._arena = A
    assert cw.ci_pad == lin_ci_pad(c), (cw.ci_pad, lin_id(c))
    if key is not None:
        LIN_PACKED[dev, key] = cw
    return cw


def lin_onehot(c, m, dev="cpu"):
    """the packed one-hot weight of column block m (value 448 for fp8: quantize_f8_cols then gives column scale exactly
    1.0 and code 448)"""
    v = 448.0 if c.kern == "f8" else 1.0
    return lin_pack(c, delta_weights(c.Co, c.Ci, 1, 0, m)[:, :, 0] * v, None, (c.kern == "f8", c.Co, c.Ci, m), dev)


def lin_make_x(c, seed=0):
    """host operand of a case -> (x as stored [B, T, Ci], x_scale [B T] | None, the staged operand the kernel must form,
    fp32: x (bf16), bf16(0.5 x) (fp32 rows, cscale 0.5: exact), code x_scale (fp8; the one-hot 448 is the caller's);
    None for a general cscale)"""
    if c.kern == "f8":
        codes, sx = e4m3_case(c.B, c.T, c.Ci, seed)
        return codes, sx, e4m3_value(codes) * sx.view(c.B, c.T, 1)
    g = torch.Generator().manual_seed(seed + c.B * c.T + c.Ci)
    x = torch.randn(c.B, c.T, c.Ci, generator=g)
    if c.idt == "bf16":
        x = bf(x)
        return x, None, x
    return x, None, bf(x * c.cscale) if c.cscale == 0.5 else None


def lin_x_layout(c, x, poisoned, dev="cpu"):
    """x on `dev` -> (buffer, Act): poisoned = channel-offset inside a wider, longer buffer of finite poison (2^100; fp8:
    the code 0x7E), bsx != T ldx; else compact and zero padded"""
    dt = LIN_DT[c.idt]
    fill = (LIN_POISON_F8 if poisoned else 0) if c.kern == "f8" else (LIN_POISON if poisoned else 0.0)
    xb, xa = guarded((c.B, c.T, c.Ci), lin_x_pads(c, poisoned), fill, dt, dev)
    if c.kern == "f8":
        xa.t.view(torch.uint8)[:, :, xa.c0:xa.c0 + c.Ci] = x.to(dev)
    else:
        xa.t[:, :, xa.c0:xa.c0 + c.Ci] = x.to(dev, dt)
    assert xa.c0 + lin_ci_pad(c) <= xa.ld and (not poisoned or xa.bs != c.T * xa.ld)
    return xb, xa


def lin_y_layout(c, poisoned, dev="cpu"):
    """the output -> (buffer, Act): NaN-sentinel filled and guarded by the case's ypads, or compact zeros"""
    dt = LIN_DT[c.odt]
    if poisoned:
        return guarded((c.B, c.T, c.Co), c.ypads, LIN_SENT[dt], dt, dev)
    return guarded((c.B, c.T, c.Co), (0, 0, 0), 0.0, dt, dev)


# ---- the precise (split-operand) convs: exact probes and exact-sum dense checks (tests/test_gpu_precise_probe.py,
# test_refops_x3.py, the --precise-cases mode of tools/dispatch_trace.py) ----
# The precise kernels (csrc/mrfx.hip mrfx_conv / mrfx_lin, csrc/convx.hip conv_x3) split every fp32 operand into hi =
# bf16(z), lo = bf16(z - hi) and form w z as wl zh + wh zl + wh zh on the bf16 MFMA with fp32 accumulation (wl zl is
# dropped).  hi + lo is exactly representable in fp32, so a one-hot weight 1.0 reads the staged PAIR out bit for bit; and
# with operands a + b 2^-10 (small integers a, |b| <= 3) every product and partial sum is a multiple of 2^-10 below 2^13:
# any accumulation order gives the same bits, equal to the fp64 sum of the three products.

PX_POISON = 2.0 ** 100          # finite: 0 * poison = 0, and mrfx_conv's x * 0 of the channels [Ci, ceil8(Ci))
PX_SENT = 0x7FC0A5A5            # the NaN payload of the output guards
PX_XPADS, PX_YPADS = (3, 8, 8), (2, 8, 8)   # guarded()'s pads: every pitch a multiple of 8 floats, 32-byte bases

# prologues: (AdaIN: None | "p2" (power-of-two sc, sh = 0) | "gen", activation, slope, exact?) -- the table of
# tests/test_gpu_conv_probe.py PRO
PX_PRO = {
    "none": (None, None, 0.0, True),
    "adain2": ("p2", None, 0.0, True),
    "adain2_leaky8": ("p2", "leaky", 0.125, True),
    "leaky8": (None, "leaky", 0.125, True),
    "leaky.1": (None, "leaky", 0.1, False),
    "leaky.01": (None, "leaky", 0.01, False),
    "adain_leaky.2": ("gen", "leaky", 0.2, False),
    "snake": ("gen", "snake", 0.0, False),
    "leaky2": (None, "leaky", 2.0, True),  # (the exact-sum launches: negative values doubled, the 2^-10 grid kept)
}


def split_ref(z):
    """fp32 -> (hi, lo, S) fp32: hi = bf16(z) to nearest even, lo = bf16(z - hi) (the difference is exact), S = hi + lo
    (exact in fp32: lo's lowest bit is not below z's)"""
    z = z.float()
    hi = z.to(torch.bfloat16).float()
    lo = (z - hi).to(torch.bfloat16).float()
    return hi, lo, hi + lo


def x3_prologue32(x, sc=None, sh=None, act=None, slope=0.0):
    """the fp32 prologue value of the exact prologues (no AdaIN: sc 1, sh 0; power-of-two AdaIN; LeakyReLU with a
    power-of-two slope): x sc + sh, then the activation, every step exact -> fp32 [B, T, C].  (-0 becomes +0: -0 + 0.)"""
    x = x.float()
    one = torch.ones(x.shape[0], x.shape[2])
    sc = one if sc is None else sc.float()
    sh = 0 * one if sh is None else sh.float()
    v = x * sc[:, None, :] + sh[:, None, :]
    if act == "leaky":
        v = torch.where(v >= 0, v, v * slope)
    else:
        assert act is None, act
    return v


def x3_identity_expect(x, sc=None, sh=None, act=None, slope=0.0):
    """what a precise conv with a one-hot weight 1.0 must read out for an exact prologue: S = hi + lo of the exact fp32
    prologue value (the kernel computes 0 + wl zh (= 0) + wh zl + wh zh) -> fp32 [B, T, C]"""
    return split_ref(x3_prologue32(x, sc, sh, act, slope))[2]


def _epilogue64(y, t, b, gate, res, res_tdiv, out_scale, acc_in, beta):
    """((y + b) gate + res) out_scale + beta acc_in on the values y and on the magnitudes t -> (y, t) fp64"""
    rep = lambda r: r.double().repeat_interleave(res_tdiv, dim=1)[:, :y.shape[1]] if res_tdiv > 1 else r.double()
    if b is not None:
        y, t = y + b.double(), t + b.double().abs()
    if gate is not None:
        y, t = y * gate.double()[:, None, :], t * gate.double().abs()[:, None, :]
    if res is not None:
        y, t = y + rep(res), t + rep(res).abs()
    y, t = y * out_scale, t * abs(out_scale)
    if acc_in is not None:
        y, t = y + beta * acc_in.double(), t + abs(beta) * acc_in.double().abs()
    return y, t


def x3_terms_ref(zh, zl, wh, wl, b, *, pad=0, dil=1, stride=1, res=None, res_tdiv=1, out_scale=1.0, acc_in=None,
                 beta=0.0, gate=None, ups=0, ups_pad=0, refl=0, lolo=False):
    """conv_terms_ref on the kernel's three products, in fp64: wl zh + wh zl + wh zh (wl zl excluded; lolo: included,
    for the self-checks), then the epilogue once.  zh / zl [B, T, Ci] the staged planes, wh / wl the weight's planes in
    the conv's (or ConvTranspose's) weight layout -> (y, terms) [B, T_out, Co] fp64, terms on absolute values."""
    kw = dict(pad=pad, dil=dil, stride=stride, ups=ups, ups_pad=ups_pad, refl=refl)
    y = t = 0.0
    for x, w in ((zh, wl), (zl, wh), (zh, wh)) + (((zl, wl),) if lolo else ()):
        yy, tt = conv_terms_ref(x, w, None, **kw)
        y, t = y + yy, t + tt
    return _epilogue64(y, t, b, gate, res, res_tdiv, out_scale, acc_in, beta)


def exact_sum_case(K, seed, *, B, T, Ci, Co, k=1, T_out=None, alpha=1.0, beta=0.0, res=False, res_tdiv=1, res_B=None,
                   acc=False, gate=False, zscale=1):
    """operands of an exact-sum launch: x [B, T, Ci] and w [Co, Ci, k] hold a + b 2^-10 with integers |a| <= 2 (<= 1
    where K = Ci k > 1408) and |b| <= 3 (b = 3 sign(a) instead of -3 sign(a) where |a| = 1), so hi = a and lo = b 2^-10; one value in
    eight is an exact zero (a = 0 never meets b != 0: hi would be b 2^-10); bias, residual and accumulate input small integers, alpha in {1, 0.5}, beta in {1, 2}, gates
    in {1, 2, -1}; zscale: the largest factor an exact prologue applies to x (2 for LeakyReLU with slope 2).  Every product (wl zl is never formed) and every partial sum in any order is then a multiple of 2^-g,
    g = 10 (11 with alpha = 0.5).  The condition of the case, asserted here on its worst case: (sum |w||z| + |bias| +
    |res| + |beta acc|) 2^g < 2^24 -- every intermediate is exactly representable in fp32.
    -> dict(x, w, b, res, acc, gate, alpha, beta)"""
    assert K == Ci * k and alpha in (1.0, 0.5) and beta in (0.0, 1.0, 2.0)
    amax = 2 if K <= 1408 else 1
    g = torch.Generator().manual_seed(seed)

    def val(*s):
        a, b = torch.randint(1, amax + 1, s, generator=g) * (2 * torch.randint(0, 2, s, generator=g) - 1), torch.randint(-3, 4, s, generator=g)
        zero = torch.randint(0, 8, s, generator=g) == 0  # exact zeros; a = 0 with b != 0 would make hi = b 2^-10 and
        a, b = a.masked_fill(zero, 0), b.masked_fill(zero, 0)  # wl zh a multiple of 2^-20: never drawn
        # (1 - 3 2^-10 lies beyond the tie 1 - 2^-9 of the binade under 1: hi would be 1 - 2^-8 and wl zh a multiple of
        # 2^-18.  There b takes a's sign.)
        b = torch.where((a.abs() == 1) & (b == -3 * a), -b, b)
        return (a + b * 2.0 ** -10).float()
    ints = lambda *s: torch.randint(-4, 5, s, generator=g).float()
    T_out = T if T_out is None else T_out
    o = dict(x=val(B, T, Ci), w=val(Co, Ci, k), b=ints(Co), alpha=alpha, beta=beta, res=None, acc=None, gate=None)
    if res:
        o["res"] = ints(B if res_B is None else res_B, (T_out + res_tdiv - 1) // res_tdiv, Co)
    if acc:
        o["acc"] = ints(B, T_out, Co)
    if gate:
        o["gate"] = torch.tensor([1.0, 2.0, -1.0])[torch.randint(0, 3, (B, Co), generator=g)]
    gr = 10 + (alpha == 0.5)
    worst = (K * zscale * (amax + 3 * 2.0 ** -10) ** 2 + 4) * (2 if gate else 1) + (4 if res else 0) + (4 * beta if acc else 0)
    assert worst * 2.0 ** gr < 2.0 ** 24, (K, worst, gr)
    assert worst / (2 if gate else 1) < 2.0 ** 13
    return o


def x3_dense_ratio(got, ref_full, terms, K):
    """a precise conv's fp32 output against ref_full = sum w S in fp64 (fp32 w, the read-out S): the largest |got - ref|
    / bound, bound = (2^-16 + 2^-17 + 2 (3K + 4) 2^-24) terms -- the dropped wl zl (2^-8 x 2^-8 relative), the weight's
    lo rounding (2^-17), and dense_ratio's accumulation constants with K -> 3K (as lstm_tf_ref's precise mode).  <= 1."""
    bound = (2.0 ** -16 + 2.0 ** -17 + 2.0 * (3 * K + 4) * 2.0 ** -24) * terms
    return ((got.double() - ref_full).abs() / bound.clamp_min(1e-300)).max().item()


def x3_staged_ratio(S, s64, mag):
    """the read-out pair S against the fp64 prologue s of an inexact prologue: the largest |S - s| / (2^-17 |s| + 2^-20
    mag) -- the split's truncation plus 16 fp32 ulps of the prologue magnitude (pro_ref64's mag) for the fp32 affine and
    the sine (v_sin_f32 on revolutions in mrfx_conv, libm sinf in conv_x3: the constant is an allowance, not derived)."""
    return ((S.double() - s64).abs() / (s64.abs() * 2.0 ** -17 + mag * 2.0 ** -20).clamp_min(1e-300)).max().item()


def x3_emulate(x, w, b=None, *, sc=None, sh=None, act=None, slope=0.0, snake_alpha=None, pad=0, dil=1, stride=1, res=None,
               res_tdiv=1, out_scale=1.0, acc_in=None, beta=0.0, gate=None, cscale=1.0, order="seq", mutate=None, ups=0,
               ups_pad=0, refl=0):
    """A value-level fp32 model of a precise conv on the CPU: the fp32 prologue (x cscale, sc / sh [B, Ci], LeakyReLU or
    Snake with torch's fp32 sine), the split, three bf16 products per term accumulated in torch.float32 in the given
    order -- "seq" tap-major sequential (per term wl zh, wh zl, wh zh), "rev" the same reversed, "blk32" 32-wide K-steps
    each as wl zh, wh zl, wh zh block sums (the MFMA order of csrc/mrfx.hip) --, then the fp32 epilogue ((acc + b) gate +
    res) out_scale + beta acc_in.  ups > 0: the polyphase ConvTranspose1d(stride ups, padding ups_pad, k = 2 ups) of
    weight w.transpose(0, 1), as a conv over the zero-stuffed staged rows with the taps reversed (a zero row adds exact
    zeros), then ReflectionPad(refl, 0).  -> (y [B, T_out, Co] fp32, S [B, T, Ci] fp32 the staged pair's sum).
    mutate, one value-only mistake for tests/test_refops_x3.py: "drop_wlzh" (wl zh missing in the second K-step),
    "lo_tap" (the lo plane of tap 0 taken at tap 1's rows), "lo_row" (staged lo row 3 taken from row 4), "lolo" (wl zl
    added), "adain_utt0" (utterance 0's AdaIN constants for every utterance), "alpha127" (Snake alpha of channel c & 127),
    "tdiv" (res_tdiv ignored)."""
    B, T, Ci = x.shape
    Co, _, k = w.shape
    f32 = torch.float32
    one = torch.ones(B, Ci)
    sc = one if sc is None else sc.to(f32)
    sh = 0 * one if sh is None else sh.to(f32)
    if mutate == "adain_utt0":
        sc, sh = sc[:1].expand(B, Ci), sh[:1].expand(B, Ci)
    v = (x.to(f32) * cscale) * sc[:, None, :] + sh[:, None, :]
    if act == "leaky":
        v = torch.where(v >= 0, v, v * slope)
    elif act == "snake":
        a = snake_alpha.to(f32)
        if mutate == "alpha127":
            a = a[torch.arange(Ci) & 127]
        v = v + torch.sin(a * v) ** 2 / a
    zh, zl, S = split_ref(v)
    wh, wl, _ = split_ref(w)
    if mutate == "lo_row":
        zl = zl.clone()
        zl[:, 3] = zl[:, 4]
    if ups:
        def stuff(z):
            u = torch.zeros(B, (T - 1) * ups + 1, Ci)
            u[:, ::ups] = z
            return u
        zh, zl, wh, wl = stuff(zh), stuff(zl), wh.flip(2), wl.flip(2)
        T, pad, dil, stride = (T - 1) * ups + 1, k - 1 - ups_pad, 1, 1
    T_out = (T + 2 * pad - dil * (k - 1) - 1) // stride + 1
    col = lambda z: torch.stack([F.pad(z, (0, 0, pad, pad))[:, j * dil:j * dil + (T_out - 1) * stride + 1:stride]
                                 for j in range(k)], 2)  # [B, To, k, Ci]
    ch, cl = col(zh), col(zl)
    if mutate == "lo_tap":
        cl = cl.clone()
        cl[:, :, 0] = cl[:, :, 1]
    ch, cl = ch.reshape(B, T_out, k * Ci), cl.reshape(B, T_out, k * Ci)
    mh, ml = (m.permute(0, 2, 1).reshape(Co, k * Ci) for m in (wh, wl))  # [Co, (tap, ci)]
    acc = torch.zeros(B, T_out, Co, dtype=f32)
    K = k * Ci
    if order == "blk32":
        for s in range(0, K, 32):
            e = min(s + 32, K)
            if not (mutate == "drop_wlzh" and s == 32):
                acc = acc + ch[:, :, s:e] @ ml[:, s:e].t()
            acc = acc + cl[:, :, s:e] @ mh[:, s:e].t()
            acc = acc + ch[:, :, s:e] @ mh[:, s:e].t()
            if mutate == "lolo":
                acc = acc + cl[:, :, s:e] @ ml[:, s:e].t()
    else:
        assert order in ("seq", "rev"), order
        for i in (range(K) if order == "seq" else range(K - 1, -1, -1)):
            if not (mutate == "drop_wlzh" and 32 <= i < 64):
                acc = acc + ch[:, :, i, None] * ml[None, None, :, i]
            acc = acc + cl[:, :, i, None] * mh[None, None, :, i]
            acc = acc + ch[:, :, i, None] * mh[None, None, :, i]
            if mutate == "lolo":
                acc = acc + cl[:, :, i, None] * ml[None, None, :, i]
    y = acc
    if refl:
        y, T_out = torch.cat([y[:, refl:2 * refl].flip(1), y], 1), T_out + refl
    if b is not None:
        y = y + b.to(f32)
    if gate is not None:
        y = y * gate.to(f32)[:, None, :]
    if res is not None:
        tr = torch.arange(T_out) // (1 if mutate == "tdiv" else res_tdiv)
        y = y + res.to(f32)[:, tr.clamp_max(res.shape[1] - 1)]
    y = y * out_scale
    if acc_in is not None:
        y = y + beta * acc_in.to(f32)
    return y, S


# kern: conv (mrfx_conv) | narrow (its conv_post form: the waves split the rows) | lin (mrfx_lin) | x3 (csrc/convx.hip
# conv_x3; ups > 0: its polyphase ConvTranspose, k = 2 ups) | x3flat (its FLAT linear form); tile: the tile height
# stzs_mrfx_conv_launch gives the case (asserted without a device by tests/test_dispatch_trace.py); pad None: "same"
PxCase = namedtuple("PxCase", "kern B T Ci Co k dil pro tile cscale stride pad ups refl",
                    defaults=(1, 1, "none", 128, 1.0, 1, None, 0, 0))


def px_id(c):
    return (f"{c.kern}-{c.B}x{c.T}-{c.Ci}to{c.Co}-k{c.k}d{c.dil}-{c.pro}-t{c.tile}" +
            (f"-cs{c.cscale}" if c.cscale != 1.0 else "") + (f"-s{c.stride}p{c.pad}" if c.stride != 1 else "") +
            (f"-ups{c.ups}r{c.refl}" if c.ups else ""))


def px_pad(c):
    return c.dil * (c.k - 1) // 2 if c.pad is None else c.pad


def px_T_out(c):
    """rows of the case's output: the conv's, or T ups + refl for the polyphase ConvTranspose"""
    return c.T * c.ups + c.refl if c.ups else (c.T + 2 * px_pad(c) - c.dil * (c.k - 1) - 1) // c.stride + 1


def precise_probe_cases():
    """the identity-probe table of tests/test_gpu_precise_probe.py: the smallest cases that reach each code path of
    csrc/mrfx.hip"""
    C, out = PxCase, []
    # single chunk, Snake, 128-row tiles: k3 d8 stages 144 = 16 SB rows exactly, k7 d5 158 of 160; T = 300 gives tile 1
    # the FULL interior staging path
    for k, d in ((3, 1), (3, 8), (7, 3), (7, 5), (11, 1)):
        out += [C("conv", 2, T, 128, 128, k, d, "snake", 128) for T in (5, 128, 129, 300)]
    for d in (3, 5):  # 64-row tiles (the k11 instantiations are the only reachable ones); T = 200: tile 1 interior
        out += [C("conv", 2, T, 128, 128, 11, d, "snake", 64) for T in (5, 64, 65, 200)]
    # multi-chunk (NCH = 0: half-group staging beside live accumulators); 384 -> 176: two output tiles, Co < co_pad
    for Ci, Co, k, d, tile in ((256, 256, 3, 1, 128), (256, 256, 7, 3, 128), (384, 176, 11, 5, 64)):
        out += [C("conv", 2, T, Ci, Co, k, d, "snake", tile) for T in (65, 200)]
    # the AdaIN-block k3 forms (the alpha != 1 template): 130 -> 64 has ci_pad 256 and one valid vector with 2 valid
    # channels in the second chunk
    for Ci, Co, pro in ((130, 64, "adain2_leaky8"), (130, 64, "adain_leaky.2"), (130, 64, "adain2"), (130, 64, "none"),
                        (264, 128, "none")):
        out += [C("conv", 2, T, Ci, Co, 3, 1, pro, 128) for T in (5, 129)]
    for pro in ("leaky8", "leaky.01"):  # conv_post: masked stores past Co = 22
        out += [C("narrow", 2, T, 128, 22, 7, 1, pro, 128) for T in (5, 128, 130)]
    # mrfx_lin: K 640 = 5 chunks (the next-chunk register prefetch), K 200 (ci_pad 256: whole vectors past Ci); rows
    # straddling utterances on a non-compact bsx, a partial last tile, T_in = 1; Co 136: 8 valid columns in the second
    # output tile
    out += [C("lin", 3, 50, K, 136) for K in (128, 256, 640, 200)]
    out += [C("lin", B, T, 256, 136) for B, T in ((1, 128), (2, 129), (64, 1))]
    out += [C("lin", 2, 129, 128, Co) for Co in (8, 600)]
    out += [C("lin", 3, 50, 200, 136, cscale=0.5)]
    # conv_x3, fp32 in and out (the only dtype pair the precise engines launch -- tools/dispatch_trace.py --synth): a k5
    # conv with every prologue instantiation (90 channels: the last vector holds 2), the FLAT k1 form with Ci 48, the
    # stride-6 k12 noise conv at T = 800 (774 staged rows: the tight row pitch), the polyphase ConvTransposes
    out += [C("x3", 2, 129, 90, 80, 5, 1, pro) for pro in ("none", "leaky8", "adain2_leaky8", "leaky.1", "snake")]
    out += [C("x3", 2, 5, 90, 80, 5, 1, "leaky8"), C("x3flat", 3, 50, 48, 136), C("x3flat", 64, 1, 48, 136)]
    out += [C("x3", 2, 800, 22, 32, 12, 1, pro, stride=6, pad=3) for pro in ("none", "snake")]
    out += [C("x3", 2, 65, 128, 64, 2 * s, 1, "leaky8", ups=s, refl=r) for s in (6, 10) for r in (0, 1)]
    out += [C("x3", 2, 65, 128, 64, 12, 1, "leaky.1", ups=6, refl=1)]
    return out


def x3_lds_bytes(rows_in):
    """csrc/convx.hip x3_lds_bytes restated: two staged tiles at the padded 80-byte row pitch, or at the tight 64-byte
    pitch where the padded ones would not fit 160 KB, + the 3-slot hi | lo weight ring + the prologue constants"""
    ring = 3 * 2 * 128 * 32 * 2 + 3 * 32 * 4
    px = 80 if 2 * ((rows_in * 80 + 15) & ~15) + ring <= 160 * 1024 else 64
    return max(2 * ((rows_in * px + 15) & ~15) + ring, 128 * 132 * 4 + 2 * 128 * 4 + 2 * 4 * 128 * 2 * 4)


def px_expected_launch(c):
    """what the case must launch: (kernel name, grid x, grid y, dynamic LDS bytes) -- stzs_mrfx_conv_launch restated"""
    co_pad = (max(c.ups, 1) * c.Co + 127) // 128 * 128
    if c.kern == "x3flat":
        return "conv_x3", (c.B * c.T + 127) // 128, co_pad // 128, x3_lds_bytes(128)
    if c.kern == "x3":  # (the ConvTranspose: two taps over T + 1 rows)
        To, k = (c.T + 1, 2) if c.ups else (px_T_out(c), c.k)
        return "conv_x3", c.B * ((To + 127) // 128), co_pad // 128, x3_lds_bytes(127 * c.stride + (k - 1) * c.dil + 1)
    if c.kern == "lin":
        return "mrfx_lin", (c.B * c.T + 127) // 128, co_pad // 128, 2 * 128 * 256
    rows_in = c.tile + (c.k - 1) * c.dil
    return ("mrfx_conv", c.B * ((c.T + c.tile - 1) // c.tile), 1 if c.kern == "narrow" else co_pad // 128,
            2 * rows_in * 256 + 2048)


def px_make_ops(c, seed=0):
    """host operands of a case: fp32 x, AdaIN statistics / gamma / beta (distinct per utterance), Snake alpha -- as
    tests/test_gpu_conv_probe.py make_ops"""
    adain, act, slope, _ = PX_PRO[c.pro]
    g = torch.Generator().manual_seed(seed)
    o = dict(x=torch.randn(c.B, c.T, c.Ci, generator=g), mean=None, alpha=None)
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


def px_consts(o):
    """(sc, sh) fp32 [B, Ci] as the kernel forms them ((1 + gamma) rstd, beta - mean sc, one fp32 rounding each), or
    (None, None) without AdaIN"""
    if o["mean"] is None:
        return None, None
    sc = (1 + o["gamma"].float()) * o["rstd"].float()
    return sc, o["beta"].float() - o["mean"].float() * sc


def px_layout(c, o, poisoned, dev="cpu"):
    """device operands of a case.  poisoned: x at channel offset 8 inside a wider (8 more columns) and longer (3 more rows
    per utterance) buffer of the finite poison 2^100, statistics / gamma-beta rows with non-compact strides; else compact
    and zero padded.  Every pitch stays a multiple of 8 floats (the launchers refuse anything else)."""
    Ci = c.Ci
    xb, xa = guarded((c.B, c.T, Ci), PX_XPADS if poisoned else (0, 0, 0), PX_POISON if poisoned else 0.0, torch.float32, dev)
    xa.t[:, :, xa.c0:xa.c0 + Ci] = o["x"].to(dev)
    d = dict(x=xa, xb=xb, pro=None, alpha=o["alpha"].to(dev) if o["alpha"] is not None else None)
    if o["mean"] is not None:
        sbs, gbs, boff = (Ci + 24, 2 * Ci + 40, Ci + 16) if poisoned else (Ci, 2 * Ci, Ci)
        fill = PX_POISON if poisoned else 0.0
        mean, rstd = (torch.full((c.B, sbs), fill, device=dev) for _ in range(2))
        gb = torch.full((c.B, gbs), fill, device=dev)
        mean[:, :Ci], rstd[:, :Ci] = o["mean"].to(dev), o["rstd"].to(dev)
        gb[:, :Ci], gb[:, boff:boff + Ci] = o["gamma"].to(dev), o["beta"].to(dev)
        d["pro"] = (mean, rstd, sbs, gb.data_ptr(), gbs, boff)
        d["keep"] = gb
    return d


def px_y(c, poisoned, dev="cpu", T_out=None):
    """the fp32 output -> (buffer, Act): NaN-sentinel filled and guarded, or compact zeros"""
    shp = (c.B, px_T_out(c) if T_out is None else T_out, c.Co)
    if poisoned:
        return guarded(shp, PX_YPADS, PX_SENT, torch.float32, dev)
    return guarded(shp, (0, 0, 0), 0.0, torch.float32, dev)


def px_operand(h, dev="cpu"):
    """a read-only epilogue operand [B, T, Co] in a guarded buffer of its own (finite poison around it; pitches that
    differ from the output's) -> (buffer, Act)"""
    buf, a = guarded(tuple(h.shape), (1, 16, 8), PX_POISON, torch.float32, dev)
    a.t[:, :, a.c0:a.c0 + h.shape[2]] = h.to(dev)
    return buf, a


PX_PACKED = {}


def px_pack(c, w, b=None, key=None, dev="cpu"):
    """pack (and cache, under `key`) w [Co, Ci, k] with its split-operand streams for the case's kernel"""
    if key is not None and (dev, key) in PX_PACKED:
        return PX_PACKED[dev, key]
    from stzs.weights import Arena, pack_conv
    A = Arena()
    cw = pack_conv(A, "t", w if c.kern != "lin" else w[:, :, 0], b, ups=c.ups, frag32=c.kern == "conv",
                   narrow32=c.kern == "narrow", x3=True)
    A.finalize(dev)
    cw.w, cw.wx3 = A[cw.w], A[cw.wx3]
    assert (cw.fx3 is None) == c.kern.startswith("x3"), px_id(c)
    cw.fx3 = A[cw.fx3] if cw.fx3 is not None else None
    cw.b = A[cw.b] if cw.b is not None else None
    cw._arena = A
    if key is not None:
        PX_PACKED[dev, key] = cw
    return cw


def px_args(eng, c, cw, d, ya, **epi):
    """the stzs_conv_args of one launch as the engine fills and routes them (eng.conv(..., collect=[])); the flag the case
    took is asserted: STZS_CONV_W_FRAG32X3 (csrc/mrfx.hip) for conv / narrow / lin, STZS_CONV_W_X3 (conv_x3) for x3 /
    x3flat"""
    from stzs import _lib as L
    _, act, slope, _ = PX_PRO[c.pro]
    grp = []
    geo = dict(ups_pad=c.ups // 2, T_final=c.T * c.ups, refl=c.refl) if c.ups else dict(pad=px_pad(c), dil=c.dil, stride=c.stride)
    eng.conv(cw, d["x"], ya, pro=d["pro"], pro_act={None: L.ACT_NONE, "leaky": L.ACT_LEAKY, "snake": L.ACT_SNAKE}[act],
             pro_slope=slope, pro_alpha=d["alpha"], cscale=c.cscale, collect=grp, what=px_id(c), **geo, **epi)
    a = grp[0]
    want, other = (L.CONV_W_X3, L.CONV_W_FRAG32X3) if c.kern.startswith("x3") else (L.CONV_W_FRAG32X3, L.CONV_W_X3)
    assert a.flags & want and not a.flags & other, (px_id(c), a.flags)
    return a


def px_launch(eng, a):
    """one stzs_conv1d call; its return code is asserted 0"""
    import ctypes
    rc = eng.lib.stzs_conv1d(ctypes.byref(a), eng.stream())
    assert rc == 0, f"stzs_conv1d returned {rc}"


def precise_exact_cases():
    """the exact-sum launches of tests/test_gpu_precise_probe.py (section c): (case, seed, epilogue) with epilogue =
    dict(res, res_tdiv, res_B, acc, alpha, beta, gate, stat) -- every non-Snake instantiation of mrfx_conv's pick_form
    and every mrfx_lin<NONE, ...> once"""
    C, out = PxCase, []
    E = lambda **kw: dict(dict(res=False, res_tdiv=1, res_B=None, acc=False, alpha=1.0, beta=0.0, gate=False, stat=False), **kw)
    # the LeakyReLU / identity k3 template, with and without residual, res_tdiv = 2 at odd T; LeakyReLU with slope 2
    for pro in ("none", "leaky2"):
        c = C("conv", 2, 129, 130, 64, 3, 1, pro, 128)
        out += [(c, 11, E(stat=True)), (c, 11, E(res=True, alpha=0.5, stat=True)),
                (c, 11, E(res=True, res_tdiv=2, alpha=0.5, stat=True))]
    # large K: 9 chunks, the last with 2 valid channels, two output tiles; |a|, |c| <= 1
    out.append((C("conv", 2, 129, 1090, 256, 3, 1, "none", 128), 12, E(res=True, res_tdiv=2, alpha=0.5, stat=True)))
    out.append((C("narrow", 2, 130, 128, 22, 7, 1, "leaky2", 128), 13, E()))  # conv_post shape
    for gate in (False, True):  # mrfx_lin: gate x residual (rows | the broadcast bsr = 0 form) x accumulate
        for res in (None, "rows", "bcast"):
            for acc in (False, True):
                out.append((C("lin", 3, 50, 256, 136), 14, E(gate=gate, res=res is not None, res_B=1 if res == "bcast" else None,
                                                              acc=acc, alpha=0.5 if acc else 1.0, beta=2.0 if acc else 0.0)))
    out.append((C("lin", 2, 129, 640, 136), 15, E(res=True)))  # 5 chunks, a partial last tile
    # conv_x3: the k5 form with the full epilogue, its LeakyReLU instantiation, the FLAT form with gate + residual, the
    # stride-6 k12 conv on the tight row pitch
    out.append((C("x3", 2, 129, 90, 80, 5, 1, "none"), 16, E(res=True, acc=True, alpha=0.5, beta=2.0, stat=True)))
    out.append((C("x3", 2, 129, 90, 80, 5, 1, "leaky2"), 16, E(stat=True)))
    out.append((C("x3flat", 3, 50, 48, 136), 17, E(gate=True, res=True)))
    out.append((C("x3", 2, 800, 22, 32, 12, 1, "none", stride=6, pad=3), 18, E(res=True, alpha=0.5)))
    # the polyphase ConvTranspose with the reflection row and a residual (the case's w [Co, Ci, k] is the ConvTranspose1d
    # weight transposed)
    out.append((C("x3", 2, 65, 128, 64, 12, 1, "leaky2", ups=6, refl=1), 19, E(res=True)))
    return out


def _px_epi_id(e):
    return (("-res" if e["res"] else "") + (f"-td{e['res_tdiv']}" if e["res_tdiv"] > 1 else "") + ("-bcast" if e["res_B"] else "") +
            ("-acc" if e["acc"] else "") + (f"-a{e['alpha']:.3g}" if e["alpha"] != 1.0 else "") + ("-gate" if e["gate"] else ""))


def px_exact_id(v):
    c, seed, e = v
    return px_id(c) + _px_epi_id(e)


def px_exact_operands(c, seed, e):
    """-> (exact_sum_case's dict, the keyword arguments of the case's prologue for x3_emulate / x3_prologue32)"""
    _, act, slope, exact = PX_PRO[c.pro]
    assert exact and PX_PRO[c.pro][0] is None
    ops = exact_sum_case(c.Ci * c.k, seed, B=c.B, T=c.T, Ci=c.Ci, Co=c.Co, k=c.k, T_out=px_T_out(c), alpha=e["alpha"], beta=e["beta"],
                         res=e["res"], res_tdiv=e["res_tdiv"], res_B=e["res_B"], acc=e["acc"], gate=e["gate"],
                         zscale=max(slope, 1.0))
    return ops, dict(act=act, slope=slope)


def px_exact_ref(c, ops, pro, e):
    """the expected output of an exact-sum launch: x3_terms_ref on the real split of the exact prologue value and of the
    weights -> fp32 [B, T, Co] (asserted to be exactly the fp64 value)"""
    zh, zl, _ = split_ref(x3_prologue32(ops["x"], None, None, pro["act"], pro["slope"]))
    wh, wl, _ = split_ref(ops["w"])
    rr = ops["res"].expand(c.B, -1, -1) if ops["res"] is not None else None
    geo = dict(pad=px_pad(c), dil=c.dil, stride=c.stride)
    if c.ups:
        wh, wl, geo = wh.transpose(0, 1), wl.transpose(0, 1), dict(ups=c.ups, ups_pad=c.ups // 2, refl=c.refl)
    ref, _ = x3_terms_ref(zh, zl, wh, wl, ops["b"], res=rr, res_tdiv=e["res_tdiv"], out_scale=e["alpha"], acc_in=ops["acc"],
                          beta=e["beta"], gate=ops["gate"], **geo)
    assert bool((ref.float().double() == ref).all())
    return ref.float()


def precise_dense_cases():
    """the random dense launches of section d: (case, epilogue) -- the Snake instantiations (residual x accumulate x alpha
    on the 128-row single-chunk form, the 64-row k11 d3 form, 256 -> 256, 384 -> 176 on 64-row tiles with Co < co_pad),
    the LeakyReLU(0.2) block conv behind a general AdaIN, and mrfx_lin with gate + residual + accumulate"""
    C, out = PxCase, []
    E = lambda **kw: dict(dict(res=False, res_tdiv=1, res_B=None, acc=False, alpha=1.0, beta=0.0, gate=False, stat=True), **kw)
    c = C("conv", 2, 300, 128, 128, 7, 3, "snake", 128)
    out += [(c, E(res=bool(r), acc=bool(a), alpha=1 / 3 if al else 1.0, beta=0.5 if a else 0.0))
            for r in (0, 1) for a in (0, 1) for al in (0, 1)]
    out.append((C("conv", 2, 200, 128, 128, 11, 3, "snake", 64), E(res=True, acc=True, alpha=1 / 3, beta=0.5)))
    out.append((C("conv", 2, 200, 256, 256, 3, 1, "snake", 128), E(res=True, alpha=0.7071)))
    out.append((C("conv", 2, 200, 384, 176, 11, 5, "snake", 64), E(res=True, alpha=0.7071)))
    out.append((C("conv", 2, 129, 130, 64, 3, 1, "adain_leaky.2", 128), E(res=True, res_tdiv=2, alpha=0.7071)))
    out.append((C("lin", 3, 50, 640, 136), E(res=True, acc=True, gate=True, alpha=0.75, beta=1.25, stat=False)))
    # conv_x3: Snake by libm sinf behind a general AdaIN, the stride-6 conv, the polyphase ConvTranspose with a residual
    out.append((C("x3", 2, 129, 90, 80, 5, 1, "snake"), E(res=True, acc=True, alpha=1 / 3, beta=0.5)))
    out.append((C("x3", 2, 800, 22, 32, 12, 1, "snake", stride=6, pad=3), E(res=True, alpha=0.7071)))
    out.append((C("x3", 2, 65, 128, 64, 12, 1, "leaky.1", ups=6, refl=1), E(res=True, stat=False)))
    return out


def px_dense_id(v):
    c, e = v
    return px_id(c) + _px_epi_id(e)


def px_dense_operands(c, e):
    """random fp32 weights, bias and epilogue operands of a dense case -> dict(w, b, res, acc, gate)"""
    g = torch.Generator().manual_seed(c.Ci + c.k + c.T)
    wshape, fan = ((c.Ci, c.Co, c.k), 2 * c.Ci) if c.ups else ((c.Co, c.Ci, c.k), c.Ci * c.k)  # (ConvTranspose1d layout)
    o = dict(w=torch.randn(*wshape, generator=g) / math.sqrt(fan), b=torch.randn(c.Co, generator=g) * 0.1,
             res=None, acc=None, gate=None)
    To = px_T_out(c)
    if e["res"]:
        o["res"] = torch.randn(c.B, (To + e["res_tdiv"] - 1) // e["res_tdiv"], c.Co, generator=g)
    if e["acc"]:
        o["acc"] = torch.randn(c.B, To, c.Co, generator=g)
    if e["gate"]:
        o["gate"] = torch.rand(c.B, c.Co, generator=g) + 0.5
    return o


def px_dense_args(eng, c, w, b, o, dev="cpu", *, res=None, res_tdiv=1, acc=None, alpha=1.0, beta=0.0, gate=None, stat=False,
                  epi_act=None):
    """the stzs_conv_args of one dense launch on the poisoned layout: res / acc_in in guarded buffers of their own (ldr,
    lda, bsr, bsa differ from ldy, bsy; a one-utterance res is the broadcast bsr = 0 form), the gate rows at a pitch
    > Co, and with stat a sentinel-filled statistics slab with stat_ld > Co and one chunk row more than the conv writes
    -> (args, dict of every buffer: x (d), y (yb, ya), res / acc (ro), gate, slab, nch)"""
    from stzs.engine import Act
    d = px_layout(c, o, True, dev)
    cw = px_pack(c, w, b, None, dev)
    ro = [px_operand(h, dev) if h is not None else (None, None) for h in (res, acc)]
    epi = dict(res=ro[0][1], res_tdiv=res_tdiv, acc_in=ro[1][1], alpha=alpha, beta=beta)
    if res is not None and res.shape[0] == 1 and c.B > 1:
        epi["res"] = Act(ro[0][1].t[:1], ro[0][1].c0, ro[0][1].C)
    if epi_act is not None:
        epi["epi_act"] = epi_act
    gd = None
    if gate is not None:
        gbs = c.Co + 24
        gd = torch.full((c.B, gbs), PX_POISON, device=dev)
        gd[:, :c.Co] = gate.to(dev)
        epi.update(gate=gd.data_ptr(), gate_bs=gbs)
    yb, ya = px_y(c, True, dev)
    a = px_args(eng, c, cw, d, ya, **epi)
    slab, nch = None, (px_T_out(c) + 63) // 64
    if stat:
        sld = (c.Co + 7) // 8 * 8 + 8
        slab = fill_bits((c.B * nch + 1, sld, 2), torch.float32, PX_SENT, dev)  # ([B][nch] rows, then the extra one)
        a.stat_part, a.stat_ld = slab.data_ptr(), sld
    return a, dict(d=d, cw=cw, yb=yb, ya=ya, ro=ro, gate=gd, slab=slab, nch=nch)


def px_dense_ref(c, S, d, e):
    """ref_full = sum w S in fp64 (fp32 w, the read-out S) with the case's epilogue, and its terms -> (ref, terms, K)"""
    geo = dict(ups=c.ups, ups_pad=c.ups // 2, refl=c.refl) if c.ups else dict(pad=px_pad(c), dil=c.dil, stride=c.stride)
    ref, terms = conv_terms_ref(S, d["w"], d["b"], res=d["res"], res_tdiv=e["res_tdiv"], out_scale=e["alpha"], acc_in=d["acc"],
                                beta=e["beta"], gate=d["gate"], **geo)
    return ref, terms, 2 * c.Ci if c.ups else c.Ci * c.k
