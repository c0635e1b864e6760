"""Why the ragged-frames masks suffice, on the CPU in fp32 on SPEC_TINY: the F0 / N predictor restated
over a zero-padded batch with the oracle's own _lin / _conv / bilstm and exactly the masks the kernels implement --

  * the shared BiLSTM per row over its own T_b frames (stzs_lstm_args.lens), zeros past them;
  * InstanceNorm statistics over each row's own rows (stzs_stats_args.lens, the fused partials' mask);
  * the rows at and past T_b (2 T_b behind the upsampling block) zeroed after each AdaIN + LeakyReLU -- what a conv with
    stzs_conv_args.t_lens stages -- and the depthwise ConvTranspose's rows >= 2 T_b zeroed (stzs_dwup_args.lens);
  * nothing else: the 1x1 shortcuts and projections run on whatever the padding holds --

against oracle.stzs_ref.f0n_predictor on every row alone.  The figure is max-abs over max|ref| of F0 and N on the row's
own 2 T_b values.  Measured with the correct recipe on the three batches below: 1.32e-6 (T40 130), 7.9e-7 (37), 8.5e-7
(12) -- the full-length row shows the same figure: the rounding of two formulations of the normalisation, not of the
padding; the bound is 4x the largest, DESIGN.md §2c's rule.  Each planted defect must leave the bound by two orders
of magnitude (they measure 0.12 .. 2.0: statistics over the padded count 0.98 / 1.97, no tail zeroing 0.81 / 0.82,
ConvTranspose tail left in place 0.12 / 0.12).  Rows of >= 3 frames
only: two samples' variance amplifies rounding to ~1e-5, and F.instance_norm rejects a 1-frame row."""
import math

import pytest
import torch
import torch.nn.functional as F

BATCHES = {"t130": [130, 65, 128, 63], "t37": [37, 9, 20, 3], "t12": [12, 5, 9, 3]}
T_TXT = 12
MEASURED = 1.32e-6
BOUND = 4 * MEASURED


def _durations(n):
    """n frames over T_TXT tokens (zeros allowed: such a token owns no frame)"""
    return [n // T_TXT + (1 if t < n % T_TXT else 0) for t in range(T_TXT)]


def _masked_adain(R, x, sg, P, name, lens, mul, defect):
    """x [B, C, T]: (1 + g) * InstanceNorm over the row's own rows + b, LeakyReLU, tail rows zeroed"""
    g, b = R._lin(sg, P, name).chunk(2, dim=1)
    out = torch.zeros_like(x)
    for i, n in enumerate(lens):
        tb = n * mul
        seg = x[i, :, :x.shape[2] if defect == "stats_padded" else tb]
        mu = seg.mean(1, keepdim=True)
        var = seg.var(1, unbiased=False, keepdim=True)
        y = (x[i] - mu) / torch.sqrt(var + 1e-5)
        y = F.leaky_relu((1 + g[i, :, None]) * y + b[i, :, None], 0.2)
        if defect != "no_tail_zero":
            y[:, tb:] = 0
        out[i] = y
    return out


def _blk(R, x, sg, P, name, lens, mul, up, defect):
    r = _masked_adain(R, x, sg, P, name + ".norm1", lens, mul, defect)
    if up:
        r = F.conv_transpose1d(r, P[name + ".pool.w"], P[name + ".pool.b"], stride=2, padding=1, output_padding=1,
                               groups=r.shape[1])
        mul = 2 * mul
        if defect != "convT_tail":
            for i, n in enumerate(lens):
                r[i, :, n * mul:] = 0
    r = R._conv(r, P, name + ".conv1", padding=1)
    r = _masked_adain(R, r, sg, P, name + ".norm2", lens, mul, defect)
    r = R._conv(r, P, name + ".conv2", padding=1)
    sc = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    if name + ".sc.w" in P:
        sc = F.conv1d(sc, P[name + ".sc.w"])
    return (r + sc) / math.sqrt(2.0), mul


def ragged_f0n(R, P, S, en, codes, lens, defect=None):
    """en [B, T40, pr_in], zeros past each row's frames -> F0, N [B, 2 T40] (rows past 2 T_b unspecified)"""
    sg = codes[:, :, S.style_ac:].mean(1)
    xs = torch.zeros(en.shape[0], en.shape[1], S.pr_hid)
    for i, n in enumerate(lens):
        xs[i, :n] = R.bilstm(en[i:i + 1, :n], P, "pr.shared")[0]
    x0 = xs.transpose(1, 2)
    out = []
    for br in ("f0", "n"):
        y, m = _blk(R, x0, sg, P, f"pr.{br}0", lens, 1, False, defect)
        y, m = _blk(R, y, sg, P, f"pr.{br}1", lens, m, True, defect)
        y, m = _blk(R, y, sg, P, f"pr.{br}2", lens, m, False, defect)
        out.append(R._conv(y, P, f"pr.{br}_proj")[:, 0])
    return out[0], out[1]


_runs = {}


def _case(name, tiny, tiny_params):
    """inputs and the per-row oracle of a batch, computed once"""
    if name not in _runs:
        from oracle import stzs_ref as R
        S, P = tiny, tiny_params
        lens = BATCHES[name]
        g = torch.Generator().manual_seed(sum(lens))
        B = len(lens)
        h = torch.randn(B, T_TXT, S.d_txt, generator=g)
        codes = torch.randn(B, S.L_s, S.code_dim, generator=g) * 0.3
        dur = torch.tensor([_durations(n) for n in lens], dtype=torch.int32)
        en = torch.zeros(B, max(lens), S.pr_in)
        ref = []
        with torch.no_grad():
            for b, n in enumerate(lens):
                pr = R.predict_prosody(P, S, h[b:b + 1], codes[b:b + 1], dur[b:b + 1])
                en[b, :n] = pr["en"][0]
                ref.append((pr["F0"][0], pr["N"][0]))
        _runs[name] = (R, en, codes, lens, ref)
    return _runs[name]


def _worst(name, tiny, tiny_params, defect=None):
    R, en, codes, lens, ref = _case(name, tiny, tiny_params)
    with torch.no_grad():
        F0, N = ragged_f0n(R, tiny_params, tiny, en, codes, lens, defect)
    worst = 0.0
    for b, n in enumerate(lens):
        for got, want in ((F0[b, :2 * n], ref[b][0]), (N[b, :2 * n], ref[b][1])):
            assert got.shape == want.shape
            worst = max(worst, ((got - want).abs().max() / want.abs().max()).item())
    return worst


@pytest.mark.parametrize("name", list(BATCHES))
def test_masked_recipe_matches_rows_alone(tiny, tiny_params, name):
    e = _worst(name, tiny, tiny_params)
    print(f"{name}: correct recipe, worst max-abs / max|ref| over rows, F0 and N = {e:.2e} (bound {BOUND:.2e})")
    assert e <= BOUND


@pytest.mark.parametrize("defect", ["stats_padded", "no_tail_zero", "convT_tail"])
@pytest.mark.parametrize("name", ["t130", "t37"])
def test_planted_defects_leave_the_bound(tiny, tiny_params, name, defect):
    e = _worst(name, tiny, tiny_params, defect)
    print(f"{name}: {defect}: {e:.2e}")
    assert e > 100 * BOUND
