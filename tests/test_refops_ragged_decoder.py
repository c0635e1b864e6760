"""Why the ragged decoder's masks suffice, on the CPU in fp32 on SPEC_TINY (the oracle has no form
restriction): the decoder restated over a padded batch with the oracle's own primitives (_lin / _conv, snake,
source_features with torch.stft, torch.istft) and exactly the masks the kernels implement --

  * the pre-blocks as §2d's blocks: InstanceNorm statistics over each row's own rows, the rows at and past T_b (2 T_b
    behind the upsampling block) zeroed after each AdaIN + LeakyReLU and after the depthwise ConvTranspose; the F0 / N
    stride-2 convs, asr_res and the shortcuts run on whatever the padding holds;
  * the harmonic source per row on its own 2 T_b F0 frames (the centre=True reflection at its own last sample), its
    rows past Tf_b zeros (stzs_source_args.lens); the noise convs run on the padded rows;
  * every ConvTranspose input zeroed past the row's rows after the LeakyReLU (stzs_conv_args.t_lens_rows = 1);
  * every MRF AdaIN over the row's own rows, every Snake output zeroed past them;
  * conv_post's input zeroed past the row's rows after its LeakyReLU; the iSTFT per row over its own Tf_b frames --

against oracle.stzs_ref.decode on every row alone, per stage: max-abs over max|ref| of gen_in, har, mrf_out0, mrf_out1,
post and wav on the row's own rows.  Frame counts [7, 3, 4, 6], once at the padded width 9 (no row full) and once at 7
(row 0 full length).  Rows of >= 3 frames only (F.instance_norm rejects one frame, two samples' variance amplifies
rounding).  The bound is 4x the largest figure the correct recipe measures here (DESIGN.md §2c's rule); each planted
defect must leave it by orders of magnitude in the stage it breaks.

Measured (correct recipe, worst row; padded width 9 / 7): gen_in 1.9e-7 / 1.9e-7, har 0 / 0, mrf_out0 7.8e-7 / 7.4e-7,
mrf_out1 1.6e-6 / 1.3e-6, post 2.0e-6 / 2.0e-6, wav 2.9e-6 / 2.7e-6.  Defects, in the stage each breaks: statistics over
the padded count 0.83 / 0.57 (mrf_out0), no zeroing after the Snake 0.36 / 0.34, har tail not zeroed 7.4e-2 / 7.2e-2,
reflection at the padded end 6.2e-2 / 3.5e-2 (har), ConvTranspose tail left 0.63 / 0.43, iSTFT at the padded Tf 2.9e-2
(wav); the table is in DESIGN.md §2e."""
import math

import pytest
import torch
import torch.nn.functional as F

LENS = [7, 3, 4, 6]
BATCHES = {"padded9": 9, "padded7": 7}
T_TXT = 12
STAGES = ("gen_in", "har", "mrf_out0", "mrf_out1", "post", "wav")
# the largest figure of the correct recipe over both batches, every stage and row, measured on the CPU (fp32); printed
# per stage by test_masked_recipe_matches_rows_alone
MEASURED = 2.89e-6
BOUND = 4 * MEASURED
DEFECTS = {"stats_padded": "mrf_out0", "no_zero_after_snake": "mrf_out0", "har_tail": "mrf_out0", "reflect_padded_end": "har",
           "convT_tail": "mrf_out0", "istft_padded": "wav"}


def _masked_adain(R, x, sg, P, name, rows, act, defect):
    """x [B, C, T]: (1 + g) * InstanceNorm over the row's own rows + b, the activation, tail rows zeroed"""
    g, b = R._lin(sg, P, name).chunk(2, dim=1)
    out = torch.zeros_like(x)
    for i, tb in enumerate(rows):
        seg = x[i, :, :x.shape[2] if defect == "stats_padded" else tb]
        mu = seg.mean(1, keepdim=True)
        var = seg.var(1, unbiased=False, keepdim=True)
        y = act(((1 + g[i, :, None]) * ((x[i] - mu) / torch.sqrt(var + 1e-5)) + b[i, :, None])[None])[0]
        if defect != "no_zero_after_snake":
            y[:, tb:] = 0
        out[i] = y
    return out


def _blk(R, x, sg, P, name, lens, mul, up):
    """a decoder AdaIN block with §2d's masks (tests/test_refops_ragged_frames.py)"""
    lrelu = lambda v: F.leaky_relu(v, 0.2)
    r = _masked_adain(R, x, sg, P, name + ".norm1", [n * mul for n in lens], lrelu, None)
    if up:
        r = F.conv_transpose1d(r, P[name + ".pool.w"], P[name + ".pool.b"], stride=2, padding=1, output_padding=1,
                               groups=r.shape[1])
        mul = 2 * mul
        for i, n in enumerate(lens):
            r[i, :, n * mul:] = 0
    r = R._conv(r, P, name + ".conv1", padding=1)
    r = _masked_adain(R, r, sg, P, name + ".norm2", [n * mul for n in lens], lrelu, None)
    r = R._conv(r, P, name + ".conv2", padding=1)
    sc = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    if name + ".sc.w" in P:
        sc = F.conv1d(sc, P[name + ".sc.w"])
    return (r + sc) / math.sqrt(2.0), mul


def ragged_decode(R, P, S, asr, F0, N, codes, seeds, lens, defect=None):
    """asr [B, T40, d_txt] (zeros past each row's frames), F0 / N [B, 2 T40] (anything finite past 2 T_b)
    -> {stage: [B, C, rows]} and wav [B, 600 T40] (zeros past 600 T_b)"""
    B, T40 = asr.shape[0], asr.shape[1]
    s = R.decoder_style(S, codes)
    tr = {}
    # ---- pre-blocks.  The F0 / N stride-2 convs take no length: output frame T_b - 1 reads rows 2 T_b - 3 .. 2 T_b - 1
    for n in lens:
        assert 2 * (n - 1) - 1 + (3 - 1) == 2 * n - 1
    Fd = R._conv(F0[:, None], P, "dec.f0_conv", stride=2, padding=1)
    Nd = R._conv(N[:, None], P, "dec.n_conv", stride=2, padding=1)
    a = asr.transpose(1, 2)
    x, m = _blk(R, torch.cat([a, Fd, Nd], 1), s, P, "dec.encode", lens, 1, False)
    ar = R._conv(a, P, "dec.asr_res")
    for i in range(4):
        x, m = _blk(R, torch.cat([x, ar, Fd, Nd], 1), s, P, f"dec.decode{i}", lens, m, i == 3)
    tr["gen_in"] = x
    # ---- harmonic source: per row on its own frames, zeros past Tf_b
    hs = S.istft_hop
    TfP = 2 * T40 * S.hop // hs + 1
    har = torch.zeros(B, 2 * S.n_bins, TfP)
    full = R.source_features(P, S, torch.nan_to_num(F0), seeds)[0] if defect in ("har_tail", "reflect_padded_end") else None
    for b, n in enumerate(lens):
        Tfb = 2 * n * S.hop // hs + 1
        if defect == "reflect_padded_end":
            har[b, :, :Tfb] = full[b, :, :Tfb]
        else:
            har[b, :, :Tfb] = R.source_features(P, S, F0[b:b + 1, :2 * n], seeds[b:b + 1])[0][0]
        if defect == "har_tail":
            har[b, :, Tfb:] = full[b, :, Tfb:]
    tr["har"] = har
    # ---- generator stages
    n_up = len(S.up_rates)
    rows = [2 * n for n in lens]
    for i in range(n_up):
        r, k = S.up_rates[i], S.up_kernels[i]
        last = i == n_up - 1
        xm = F.leaky_relu(x, 0.1)
        if defect != "convT_tail":
            for b, tb in enumerate(rows):
                xm[b, :, tb:] = 0
        if not last:
            sf0 = int(math.prod(S.up_rates[i + 1:]))
            xs = R._conv(har, P, f"gen.noise_conv{i}", stride=sf0, padding=(sf0 + 1) // 2)
        else:
            xs = R._conv(har, P, f"gen.noise_conv{i}")
        xu = F.conv_transpose1d(xm, P[f"gen.ups{i}.w"], P[f"gen.ups{i}.b"], stride=r, padding=(k - r) // 2)
        if last:
            xu = F.pad(xu, (1, 0), mode="reflect")
        x = xu + xs
        rows = [tb * r + (1 if last else 0) for tb in rows]
        acc = None
        for j, kr in enumerate(S.rb_kernels):
            y = x
            for mm, dil in enumerate(S.rb_dils):
                p = f"gen.rb{i}.{j}.{mm}"
                t = _masked_adain(R, y, s, P, p + ".n1", rows, lambda v: R.snake(v, P[p + ".alpha1"]), defect)
                t = R._conv(t, P, p + ".c1", dilation=dil, padding=dil * (kr - 1) // 2)
                t = _masked_adain(R, t, s, P, p + ".n2", rows, lambda v: R.snake(v, P[p + ".alpha2"]), defect)
                t = R._conv(t, P, p + ".c2", padding=(kr - 1) // 2)
                y = t + y
            acc = y if acc is None else acc + y
        x = acc / len(S.rb_kernels)
        tr[f"mrf_out{i}"] = x
    # ---- conv_post on zero padding past the row's rows, the iSTFT per row over its own frames
    xm = F.leaky_relu(x, 0.01)
    for b, tb in enumerate(rows):
        xm[b, :, tb:] = 0
    post = R._conv(xm, P, "gen.conv_post", padding=3)
    tr["post"] = post
    nb = S.n_bins
    win = torch.hann_window(S.n_fft)
    wav = torch.zeros(B, (TfP - 1) * hs)
    for b, tb in enumerate(rows):
        pb = torch.nan_to_num(post[b:b + 1]) if defect == "istft_padded" else post[b:b + 1, :, :tb]
        spec = torch.exp(pb[:, :nb]) * torch.exp(1j * torch.sin(pb[:, nb:]))
        w = torch.istft(spec, S.n_fft, hop_length=hs, win_length=S.n_fft, window=win)[0]
        wav[b, :(tb - 1) * hs] = w[:(tb - 1) * hs]
    tr["wav"] = wav[:, None]
    return tr


_runs = {}


def _case(name, tiny, tiny_params):
    """inputs of a padded batch and every row's solo oracle trace, computed once"""
    if name not in _runs:
        from oracle import stzs_ref as R
        S, P = tiny, tiny_params
        T40 = BATCHES[name]
        g = torch.Generator().manual_seed(17)
        B = len(LENS)
        h = torch.randn(B, T_TXT, S.d_txt, generator=g)
        codes = torch.randn(B, S.L_s, S.code_dim, generator=g) * 0.3
        asr = torch.zeros(B, T40, S.d_txt)
        # (what lies past a row's frames: finite values a correct recipe must not depend on)
        F0 = torch.rand(B, 2 * T40, generator=g) * 200 + 60
        N = torch.randn(B, 2 * T40, generator=g)
        seeds = [5, 6, 7, 8]
        ref = []
        with torch.no_grad():
            for b, n in enumerate(LENS):
                dur = torch.tensor([[n // T_TXT + (1 if t < n % T_TXT else 0) for t in range(T_TXT)]], dtype=torch.int32)
                pr = R.predict_prosody(P, S, h[b:b + 1], codes[b:b + 1], dur)
                asr[b, :n] = pr["asr"][0]
                F0[b, :2 * n], N[b, :2 * n] = pr["F0"][0], pr["N"][0]
                t1 = {}
                w = R.decode(P, S, asr[b:b + 1, :n], F0[b:b + 1, :2 * n], N[b:b + 1, :2 * n], codes[b:b + 1], seeds[b:b + 1], t1)
                t1["wav"] = w[:, None]
                ref.append(t1)
        _runs[name] = (R, asr, F0, N, codes, seeds, ref)
    return _runs[name]


def _errors(name, tiny, tiny_params, defect=None):
    """{stage: worst max-abs / max|ref| over the rows, on each row's own rows}"""
    R, asr, F0, N, codes, seeds, ref = _case(name, tiny, tiny_params)
    with torch.no_grad():
        tr = ragged_decode(R, tiny_params, tiny, asr, F0, N, codes, seeds, LENS, defect)
    out = {}
    for k in STAGES:
        worst = 0.0
        for b in range(len(LENS)):
            want = ref[b][k][0]
            got = tr[k][b, :, :want.shape[1]]
            assert got.shape == want.shape, (k, got.shape, want.shape)
            worst = max(worst, ((got - want).abs().max() / want.abs().max()).item())
        out[k] = worst
    return out


@pytest.mark.parametrize("name", list(BATCHES))
def test_masked_recipe_matches_rows_alone(tiny, tiny_params, name):
    e = _errors(name, tiny, tiny_params)
    print(f"{name}: correct recipe: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"  (bound {BOUND:.2e})")
    assert max(e.values()) <= BOUND, e


@pytest.mark.parametrize("defect", list(DEFECTS))
@pytest.mark.parametrize("name", list(BATCHES))
def test_planted_defects_leave_the_bound(tiny, tiny_params, name, defect):
    e = _errors(name, tiny, tiny_params, defect)
    print(f"{name}: {defect}: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e[DEFECTS[defect]] > 100 * BOUND, (defect, e)


def test_waveform_tail_is_zero(tiny, tiny_params):
    R, asr, F0, N, codes, seeds, _ = _case("padded9", tiny, tiny_params)
    with torch.no_grad():
        wav = ragged_decode(R, tiny_params, tiny, asr, F0, N, codes, seeds, LENS)["wav"][:, 0]
    for b, n in enumerate(LENS):
        assert bool((wav[b, tiny.frame40 * n:] == 0).all())
