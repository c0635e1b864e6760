"""The waveform back end (csrc/source.hip, csrc/istft.hip) and the integer path of csrc/prosody.hip (durations,
alignment, row gather), straight through the C ABI, per element against the fp64 references of tests/refops.py
(checked on the CPU by tests/test_refops_backend.py).

Every destination lies inside a larger sentinel-filled buffer (cells before it, behind every row block and between
utterances) whose cells outside the documented output must keep their bits; inputs whose leading dimension exceeds
their width carry NaN in the padding.  The accuracy constants E_SIN, E_BM (source.hip) and E_T (istft.hip) are the
kernels' own claims; every ratio printed is |kernel - fp64 reference| / bound.

One-line defects planted in scratch copies of the kernels, each run once on MI355X under this file (failed of 104) and
under the suite's earlier tests of these kernels (test_gpu_ops, test_gpu_stream without its 30-s cases, test_gpu_golden,
test_gpu_stages, test_gpu_configs: failed of 177):
    source   in-frame phase fmaf(jj, fi[h], fp[h])            12 red here    0 there (what the compiler made of the
                                                                             kernel until add_mul_2r)
             F[k] >= voiced_thr                               29             0
             noise counter from the unreflected index         36             0
             right reflection 2 N - 1 - n                     36             1
             ph0 != 0 for harmonic 0                          34             15
    iSTFT    Nyquist sign dropped                             24             17
             m > m_end                                        32             not run (unguarded buffers there)
             low constant of the range reduction removed      16             1
             halo_of with floor division                      not run on the GPU (it reads LDS in front of the
                                                              workgroup's frames); red in test_refops_backend.py
    align    cs[mid] < f                                      6              11"""
import ctypes as C

import numpy as np
import pytest
import torch

from refops import (DUR_NBINS, DUR_ROWS, ISTFT_GEOMS, SHIPPED, _ordered, align_ref, dur_logits, dur_tie_width,
                    durations_ref, f0_case, istft_bound, istft_ref, merge_weights, phase_prefix_ref, post_case, same_bits,
                    source_bound, source_ref, ulp_dist)

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -777.0
G = 16  # guard cells before and behind a destination
SEEDS = (0, 11, 0x80000000, 0xFFFFFFFF)


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


class _Dest:
    """a flat sentinel-filled device buffer around B row blocks of `n` cells at stride `bs`, G cells in front"""

    def __init__(self, B, n, bs, dtype, dev, sent=SENT):
        assert bs >= n
        self.B, self.n, self.bs = B, n, bs
        self.t = torch.full((G + B * bs + G,), sent, dtype=dtype, device=dev)
        self.before = self.t.clone()
        self.may = torch.zeros(self.t.shape, dtype=torch.bool, device=dev)
        for b in range(B):
            self.may[G + b * bs:G + b * bs + n] = True

    @property
    def ptr(self):
        return self.t.data_ptr() + G * self.t.element_size()

    def untouched(self):
        return same_bits(self.t[~self.may], self.before[~self.may])

    def rows(self):
        """the B written blocks [B, n] on the host"""
        return torch.stack([self.t[G + b * self.bs:G + b * self.bs + self.n] for b in range(self.B)]).cpu()


def _dev(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


# ---- stzs_harmonic_source --------------------------------------------------------------------------------------------

def _source(lib, f0, seeds, mw, par, nh, dtype, *, ldh=None, want=0):
    """one launch -> (har [B, Tf, ldh] on the host, prefix [B, nh, T80] fp32, guards intact).  f0 rows at ldf = T80 + 3
    with NaN padding and one NaN row behind; har at ldh = 2 nb + 3 by default, two guard rows behind every utterance
    and 7 more cells between utterances."""
    lb, L, dev = lib
    B, T80 = f0.shape
    nb = par["n_fft"] // 2 + 1
    Tf = T80 * par["hop"] // par["hop_s"] + 1
    ldf = T80 + 3
    fd = np.full((B + 1, ldf), NAN, np.float32)
    fd[:B, :T80] = f0
    fd = _dev(fd, dev)
    sd = _dev(np.array(seeds, np.uint32).view(np.int32), dev)
    wd = _dev(np.asarray(mw, np.float32), dev)
    ldh = 2 * nb + 3 if ldh is None else ldh
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    har = _Dest(B, Tf * max(ldh, 1), (Tf + 2) * max(ldh, 1) + 7, dt, dev)
    pre = _Dest(1, B * nh * T80, B * nh * T80, torch.float32, dev)
    a = L.SourceArgs()
    a.f0, a.seeds, a.merge_w, a.prefix, a.har = fd.data_ptr(), sd.data_ptr(), wd.data_ptr(), pre.ptr, har.ptr
    a.ldf, a.ldh, a.bsh = ldf, ldh, har.bs
    a.B, a.T80, a.hop, a.n_fft, a.hop_s, a.nh = B, T80, par["hop"], par["n_fft"], par["hop_s"], nh
    a.sr, a.sine_amp, a.noise_std, a.voiced_thr = par["sr"], par["sine_amp"], par["noise_std"], par["voiced_thr"]
    a.har_dtype = L.BF16 if dtype == "bf16" else L.F32
    rc = lb.stzs_harmonic_source(a, None)
    torch.cuda.synchronize()
    assert rc == want, (rc, want)
    if want != 0:  # refused: nothing ran, both destinations keep every bit
        return same_bits(har.t, har.before) and same_bits(pre.t, pre.before)
    return har.rows().view(B, Tf, ldh), pre.rows().view(B, nh, T80), har.untouched() and pre.untouched()


def _check_source(lib, f0, seeds, mw, par, nh, frames=None, what=""):
    """both har_dtype against source_ref -> (worst fp32 ratio, share of bf16 elements whose bound straddles a rounding
    boundary).  fp32: |got - ref| <= d A1 + (n_fft + 4) 2^-24 A2 per element (refops.source_bound).  bf16: the
    rounding of a value within that bound of the reference, i.e. between bf16(ref - bound) and bf16(ref + bound) --
    exactly bf16(ref) unless the bound straddles a rounding boundary (the share of such elements is printed: the
    small high-frequency bins of a smooth signal, whose bf16 ulp is of the bound's size, are most of them)."""
    nb = par["n_fft"] // 2 + 1
    ref = source_ref(f0, seeds, mw, nh=nh, frames=frames, **par)
    bound = source_bound(ref, mw, n_fft=par["n_fft"], sine_amp=par["sine_amp"], noise_std=par["noise_std"])
    sel = slice(None) if frames is None else torch.as_tensor(frames)
    want_pre = phase_prefix_ref(f0, nh, par["hop"], par["sr"]).astype(np.float32)
    out = {}
    for dtype in ("f32", "bf16"):
        har, pre, ok = _source(lib, f0, seeds, mw, par, nh, dtype)
        assert ok, f"{what} {dtype}: guard cells written"
        assert np.array_equal(pre.numpy().view(np.int32), want_pre.view(np.int32)), f"{what} {dtype}: phase prefix"
        assert bool((har[:, :, 2 * nb:].float() == 0).all()), f"{what} {dtype}: columns [2 nb, ldh) not zero"
        got = har[:, sel, :2 * nb].contiguous()
        assert bool(torch.isfinite(got.float()).all())
        if dtype == "f32":
            ratio = np.abs(got.double().numpy() - ref["bins"]) / bound
            out["ratio"] = float(ratio.max())
        else:
            lo = torch.from_numpy(ref["bins"] - bound * (1 + 1e-6)).float().to(torch.bfloat16)
            hi = torch.from_numpy(ref["bins"] + bound * (1 + 1e-6)).float().to(torch.bfloat16)
            mid = torch.from_numpy(ref["bins"]).float().to(torch.bfloat16)
            o = _ordered(got)
            inside = (o >= _ordered(lo)) & (o <= _ordered(hi))
            strad = _ordered(lo) != _ordered(hi)
            out["straddle"] = float(strad.double().mean())
            out["ulp"] = int(ulp_dist(got, mid)[~strad].max()) if bool((~strad).any()) else 0
            assert out["ulp"] <= 1
            assert bool(inside.all()), f"{what}: bf16 outside the rounding of ref +- bound at {inside.logical_not().nonzero()[0].tolist()}"
    print(f"source {what}: fp32 worst ratio {out['ratio']:.3f}; bf16 {out['ulp']} ulp from bf16(ref) where the bound "
          f"straddles no rounding boundary ({100 * out['straddle']:.1f} % of the elements' bounds do)")
    assert out["ratio"] <= 1.0, f"{what}: fp32 ratio {out['ratio']:.3f}"
    return out


def _seeds(B, i):
    return [SEEDS[(i + b) % 4] for b in range(B)]


@pytest.mark.parametrize("nh", [1, 9, 12])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T80", [1, 2, 13, 64])
def test_source_shipped_geometry(lib, T80, B, nh):
    """n_fft 20 / hop_s 5 / hop 300 (source_stft_kernel<20>).  T80 = 64: Tf = 3841, the last workgroup owns exactly the
    last frame.
    (MI355X: worst fp32 ratio 0.17 of the bound over these cases, 0.10 over every other source case of this file; bf16
    equal to bf16(ref) wherever the bound straddles no rounding boundary, which it does for 19 .. 73 % of a case's
    elements.  Measured per sample through the inverse transform of the bins: the sine within 1.9e-7 at phases below a
    cycle, Box-Muller within 1.3e-6.  FINDING: before csrc/source.hip kept the in-frame phase's product and sum apart
    (add_mul_2r) the compiler fused them into one FMA, about 2 % of the samples had a phase one fp32 ulp of t off the
    oracle's -- 3e-6 of a sine at 400 Hz, 6e-6 at 900 Hz -- and nine of these cases, the eight-row case and 20 / 3 / 300
    exceeded the bound, the worst at 1.87.)"""
    f0 = f0_case(B, T80, SHIPPED["voiced_thr"], ("shipped", T80, B, nh))
    _check_source(lib, f0, _seeds(B, T80 + nh), merge_weights(nh), SHIPPED, nh, what=f"20/5/300 T80={T80} B={B} nh={nh}")


def test_source_all_eight_frame_rows(lib):
    """hop 185 at 20 / 5: the smallest hop the host check admits, 1295 samples of a workgroup over eight 80-fps frames
    (all KW rows of the LDS tables); sr scaled with the hop so that the phase increments are those of the shipped
    geometry"""
    par = dict(SHIPPED, hop=185, sr=14800.0)
    f0 = f0_case(2, 16, par["voiced_thr"], "kw8")
    _check_source(lib, f0, [0xFFFFFFFF, 0], merge_weights(9), par, 9, what="20/5/185 T80=16")


RUNTIME_GEOMS = [(16, 4, 240, 19200.0), (32, 8, 480, 38400.0), (64, 16, 960, 76800.0), (20, 3, 300, 24000.0)]


@pytest.mark.parametrize("T80", [5, 64])
@pytest.mark.parametrize("n_fft,hop_s,hop,sr", RUNTIME_GEOMS)
def test_source_runtime_size_path(lib, n_fft, hop_s, hop, sr, T80):
    """source_stft_kernel<0> (every n_fft but 20).  T80 = 64 makes Tf - 1 a multiple of 256 in all four geometries: the
    last workgroup owns the last frame alone"""
    par = dict(SHIPPED, n_fft=n_fft, hop_s=hop_s, hop=hop, sr=sr)
    assert T80 != 64 or (T80 * hop // hop_s) % 256 == 0
    f0 = f0_case(2, T80, par["voiced_thr"], ("rt", n_fft, hop_s, T80))
    _check_source(lib, f0, _seeds(2, n_fft + T80), merge_weights(9), par, 9, what=f"{n_fft}/{hop_s}/{hop} T80={T80}")


@pytest.mark.parametrize("T80", [1024, 1025, 2049])
def test_source_long_rows_cross_the_prefix_chunk(lib, T80):
    """phase_prefix_kernel's PP_CHUNK = 1024 frames: one chunk exactly, one frame into the second, one into the third.
    The prefix of every frame is compared in bits; the bins of the first and the last 300 STFT frames against the
    reference"""
    f0 = f0_case(1, T80, SHIPPED["voiced_thr"], ("long", T80))
    Tf = T80 * 60 + 1
    frames = np.r_[0:300, Tf - 300:Tf]
    _check_source(lib, f0, [SEEDS[T80 % 4]], merge_weights(9), SHIPPED, 9, frames=frames, what=f"20/5/300 T80={T80}")


def test_source_rows_do_not_depend_on_the_batch(lib):
    """row b of a B = 3 launch equals, in bits, the B = 1 launch of that row with its seed (both dtypes)"""
    f0 = f0_case(3, 13, SHIPPED["voiced_thr"], "batch")
    seeds, mw = [0x80000000, 11, 0xFFFFFFFF], merge_weights(9)
    for dtype in ("f32", "bf16"):
        har3, _, ok = _source(lib, f0, seeds, mw, SHIPPED, 9, dtype)
        assert ok
        for b in range(3):
            har1, _, ok = _source(lib, f0[b:b + 1], seeds[b:b + 1], mw, SHIPPED, 9, dtype)
            assert ok and same_bits(har3[b:b + 1].contiguous(), har1), (dtype, b)


@pytest.mark.parametrize("s0,s1", [(0, 0x80000000), (11, 0xFFFFFFFF)])
def test_source_seeds_matter(lib, s0, s1):
    """the same F0 under two seeds (one pair differs in the top bit alone): the fp32 bins differ in frames that lie in a
    voiced stretch (noise of std 0.003 beside the sine, which bf16 would hide) and in an unvoiced one"""
    T80 = 13
    f0 = np.full((1, T80), 200.0, np.float32)
    f0[0, 6:] = 0.0
    mw = merge_weights(9)
    a, _, _ = _source(lib, f0, [s0], mw, SHIPPED, 9, "f32")
    b, _, _ = _source(lib, f0, [s1], mw, SHIPPED, 9, "f32")
    voiced, unvoiced = slice(60 + 2, 6 * 60 - 2), slice(6 * 60 + 2, 13 * 60 - 2)  # frames clear of the stretch's ends
    for name, fr in (("voiced", voiced), ("unvoiced", unvoiced)):
        differ = (a[0, fr, :22] != b[0, fr, :22]).double().mean().item()
        print(f"seeds {s0:#x} / {s1:#x}, {name} frames: {100 * differ:.1f} % of the bins differ")
        assert differ > 0.8, (name, differ)  # (the imaginary part of DC is 0 under every seed)


def test_source_refusals_launch_nothing(lib):
    """STZS_ESHAPE for hop 184 (nine 80-fps frames under one workgroup), nh 65, ldh 2 nb - 1 -- and neither the prefix
    workspace nor har has been written: every shape check runs before the first launch"""
    lb, L, dev = lib
    f0 = f0_case(1, 13, SHIPPED["voiced_thr"], "refuse")
    assert _source(lib, f0, [0], merge_weights(9), dict(SHIPPED, hop=184), 9, "f32", want=L.ESHAPE)
    assert _source(lib, f0, [0], merge_weights(65), SHIPPED, 65, "f32", want=L.ESHAPE)
    assert _source(lib, f0, [0], merge_weights(9), SHIPPED, 9, "f32", ldh=21, want=L.ESHAPE)
    assert _source(lib, f0, [0], merge_weights(9), SHIPPED, 9, "bf16", ldh=21, want=L.ESHAPE)


# ---- stzs_istft / stzs_istft_stream ---------------------------------------------------------------------------------

def _tf_set(halo):
    FB = 256 - halo
    return sorted({2, 3, halo + 1, FB, FB + 1, 2 * FB + 1, 601})


def _istft(lib, post, n_fft, hop_s):
    """whole-utterance launch of post [B, Tf, ldp] (NaN padded) at bsp = Tf ldp + 11 -> (wav [B, (Tf - 1) hop_s], _Dest)"""
    lb, L, dev = lib
    B, Tf, ldp = post.shape
    bsp = Tf * ldp + 11
    pd = np.full((B, bsp), NAN, np.float32)
    pd[:, :Tf * ldp] = post.reshape(B, -1)
    pd = _dev(pd, dev)
    n = (Tf - 1) * hop_s
    wav = _Dest(B, n, n + 9, torch.float32, dev)
    a = L.IstftArgs()
    a.post, a.wav, a.ldp, a.bsp, a.bsw = pd.data_ptr(), wav.ptr, ldp, bsp, wav.bs
    a.B, a.Tf, a.n_fft, a.hop_s = B, Tf, n_fft, hop_s
    L.check(lb.stzs_istft(a, None), "istft")
    torch.cuda.synchronize()
    return wav.rows(), wav


@pytest.mark.parametrize("cls", ["small", "mid", "large"])
@pytest.mark.parametrize("n_fft,hop_s", sorted(ISTFT_GEOMS))
def test_istft_per_sample(lib, n_fft, hop_s, cls):
    """every sample within (E_T + (nb + halo + 6) 2^-24) S of istft_ref (refops.istft_bound), E_T = 3e-6 for the three
    chained hardware transcendentals; the large-argument class (phase arguments up to +-2^17) adds E_RR = 2^-22 for the
    two roundings of the two-constant range reduction at |xr| < 4 (an fp32 ulp there is 2^-22, half of it per rounding;
    sin, cos and the magnitude carry d xr on with slope <= 1).  The
    first and last n_fft / 2 samples of a row (smallest envelope, fewest frames) are reported apart from the interior.
    Exactly (Tf - 1) hop_s samples per row are written, all finite; the guards keep their bits.
    (MI355X: worst ratio 0.087 in the edge samples (20 / 10, small) and 0.081 in the interior (20 / 4, mid) over the 24
    geometry x class cases; the large class at most 0.072 / 0.071.)"""
    halo = ISTFT_GEOMS[(n_fft, hop_s)]
    worst_edge = worst_in = 0.0
    for Tf in _tf_set(halo):
        post = post_case(2, Tf, n_fft, cls, (n_fft, hop_s, Tf, cls))
        ref, S, env = istft_ref(post, n_fft, hop_s)
        got, dest = _istft(lib, post, n_fft, hop_s)
        assert dest.untouched(), f"Tf={Tf}: guard cells written"
        assert bool(torch.isfinite(got).all()) and not bool((got == SENT).any()), f"Tf={Tf}: a sample not written"
        ratio = np.abs(got.double().numpy() - ref) / istft_bound(S, n_fft, hop_s, cls == "large")
        edge = np.zeros(ratio.shape[1], bool)
        edge[:n_fft // 2] = edge[-(n_fft // 2):] = True
        worst_edge = max(worst_edge, float(ratio[:, edge].max()))
        if (~edge).any():
            worst_in = max(worst_in, float(ratio[:, ~edge].max()))
        assert ratio.max() <= 1.0, f"Tf={Tf}: ratio {ratio.max():.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    print(f"istft {n_fft}/{hop_s} {cls}: worst ratio {worst_edge:.3f} in the edge samples, {worst_in:.3f} in the interior")


def _chunkings(Tf, halo):
    FB = 256 - halo
    out = [[2, Tf - 2]] if Tf > 2 else []
    out.append([Tf - 1, 1])
    if halo >= 2 and Tf > halo:
        out.append([halo - 1, 1, Tf - halo])
    if Tf == 2 * FB + 1:
        out.append([FB, FB, 1])
    if Tf <= FB + 1:
        out.append([1] * Tf)
    return out


@pytest.mark.parametrize("n_fft,hop_s", sorted(ISTFT_GEOMS))
def test_istft_stream_equals_whole_in_bits(lib, n_fft, hop_s):
    """stzs_istft_stream over chunkings ([1] * Tf, [halo - 1, 1, rest], [FB, FB, 1], [2, rest], a one-frame final
    chunk) writes, chunk by chunk into the range stzs_istft_stream_span names, exactly the bits of stzs_istft.  The
    tails are [B, halo, ldt] with ldt = n_fft + 5, start as NaN and alternate between calls; after each call the
    sentinel cells behind its range are checked, after the last one every guard."""
    lb, L, dev = lib
    halo = ISTFT_GEOMS[(n_fft, hop_s)]
    B, ldt = 2, n_fft + 5
    n0, n1 = C.c_int64(), C.c_int64()
    for i, Tf in enumerate(_tf_set(halo)):
        post = post_case(B, Tf, n_fft, ("small", "mid", "large")[i % 3], (n_fft, hop_s, Tf, "stream"))
        whole, _ = _istft(lib, post, n_fft, hop_s)
        ldp = post.shape[2]
        n = (Tf - 1) * hop_s
        for chunks in _chunkings(Tf, halo):
            assert sum(chunks) == Tf and min(chunks) >= 1, chunks
            wav = _Dest(B, n, n + 9, torch.float32, dev)
            tails = [torch.full((B, max(halo, 1), ldt), NAN, device=dev) for _ in range(2)]
            f0 = 0
            for j, Fc in enumerate(chunks):
                final = int(j == len(chunks) - 1)
                assert lb.stzs_istft_stream_span(f0, Fc, final, n_fft, hop_s, C.byref(n0), C.byref(n1)) == halo
                bsp = Fc * ldp + 11
                pd = np.full((B, bsp), NAN, np.float32)
                pd[:, :Fc * ldp] = post[:, f0:f0 + Fc].reshape(B, -1)
                pd = _dev(pd, dev)
                a = L.IstftStreamArgs()
                a.post, a.wav = pd.data_ptr(), wav.ptr + 4 * n0.value
                a.tail_in, a.tail_out = tails[j % 2].data_ptr(), tails[(j + 1) % 2].data_ptr()
                a.ldp, a.bsp, a.bsw, a.ldt = ldp, bsp, wav.bs, ldt
                a.B, a.f0, a.Fc, a.final_chunk, a.n_fft, a.hop_s = B, f0, Fc, final, n_fft, hop_s
                L.check(lb.stzs_istft_stream(a, None), "istft_stream")
                behind = wav.t[G + n1.value:G + n]
                assert bool((behind == SENT).all()), f"Tf={Tf} {chunks[:4]}: chunk {j} wrote past its span"
                f0 += Fc
            torch.cuda.synchronize()
            assert n1.value == n
            assert wav.untouched(), f"Tf={Tf} {chunks[:4]}: guard cells written"
            assert same_bits(wav.rows(), whole), f"Tf={Tf} chunks {chunks[:4]}..: differs from the whole-utterance call"


# ---- stzs_durations ---------------------------------------------------------------------------------------------------

def _durations(lib, logits, override=None):
    """logits [B, T, nbins] at ldl = nbins + 3, bsl = T ldl + 5 (NaN padded) -> (dur [B T] int32, dsum [B T] fp32)"""
    lb, L, dev = lib
    B, T, nbins = logits.shape
    ldl = nbins + 3
    bsl = T * ldl + 5
    ld = np.full((B, bsl), NAN, np.float32)
    for b in range(B):
        ld[b, :T * ldl].reshape(T, ldl)[:, :nbins] = logits[b]
    ld = _dev(ld, dev)
    dur = _Dest(1, B * T, B * T, torch.int32, dev, sent=-777)
    ds = _Dest(1, B * T, B * T, torch.float32, dev)
    ov = None if override is None else _dev(np.asarray(override, np.int32), dev)
    a = L.DurArgs()
    a.logits, a.override_dur, a.dur, a.dsum = ld.data_ptr(), None if ov is None else ov.data_ptr(), dur.ptr, ds.ptr
    a.ldl, a.bsl, a.B, a.T, a.nbins = ldl, bsl, B, T, nbins
    L.check(lb.stzs_durations(a, None), "durations")
    torch.cuda.synchronize()
    assert dur.untouched() and ds.untouched()
    return dur.rows()[0].numpy(), ds.rows()[0].numpy()


_DUR_SHAPES = {1: (1, 1), 255: (3, 85), 256: (2, 128), 257: (1, 257)}  # B * T -> (B, T)


@pytest.mark.parametrize("rows", DUR_ROWS)
@pytest.mark.parametrize("nbins", DUR_NBINS)
def test_durations_against_fp64(lib, nbins, rows):
    """dur = max(1, round(sum_j sigmoid)) equals the fp64 durations_ref except where the fp64 sum lies within nbins *
    2^-23 * nbins of a half-integer (an fp32 serial sum of nbins sigmoids is that close to the fp64 one); dsum is
    within the same width of the fp64 sum; such elements stay under 1 % over a bin count's four shapes (checked on
    the reference alone in test_refops_backend.py).  nbins 7 / 8 / 9 / 50 around the unrolled-by-8 loop and its tail,
    B * T 255 / 256 / 257 around one workgroup.
    (MI355X: no duration differs in any case; |dsum - fp64| at most 0.67 of the width at one bin, 0.12 at 7 .. 9 bins,
    0.04 at 50.)"""
    B, T = _DUR_SHAPES[rows]
    logits = dur_logits(rows, nbins).reshape(B, T, nbins)
    want, s64, dist = durations_ref(logits)
    dur, ds = _durations(lib, logits)
    width = dur_tie_width(nbins)
    differ = dur != want.reshape(-1)
    print(f"durations nbins={nbins} B*T={rows}: {int(differ.sum())} differ; max |dsum - fp64| = "
          f"{np.abs(ds - s64.reshape(-1)).max():.2e} (width {width:.2e})")
    assert not (differ & (dist.reshape(-1) > width)).any()
    assert (np.abs(ds.astype(np.float64) - s64.reshape(-1)) <= width).all()


def test_durations_override_and_clamps(lib):
    """override_dur (zeros included) is taken as it is; logits of +100 give exactly nbins, of -100 exactly the clamp 1"""
    g = np.random.default_rng(3)
    B, T, nbins = 2, 37, 9
    logits = g.normal(0, 2, (B, T, nbins)).astype(np.float32)
    ov = g.integers(0, 4, (B, T)).astype(np.int32)
    ov[0, 0] = ov[0, 17] = ov[1, T - 1] = 0
    dur, _ = _durations(lib, logits, ov)
    assert np.array_equal(dur, ov.reshape(-1))
    for nbins in (7, 8, 50):
        logits = np.full((1, 4, nbins), 100.0, np.float32)
        logits[0, 2:] = -100.0
        dur, ds = _durations(lib, logits)
        assert dur.tolist() == [nbins, nbins, 1, 1] and ds.tolist()[:2] == [float(nbins)] * 2 and abs(ds[2]) < 1e-30


# ---- stzs_alignment ---------------------------------------------------------------------------------------------------

def _alignment(lib, dur, T40, want=0):
    lb, L, dev = lib
    B, T = dur.shape
    dd = _dev(np.asarray(dur, np.int32), dev)
    idx = _Dest(1, B * T40, B * T40, torch.int32, dev, sent=-777)
    tot = _Dest(1, B, B, torch.int32, dev, sent=-777)
    a = L.AlignArgs()
    a.dur, a.idx, a.total, a.B, a.T, a.T40 = dd.data_ptr(), idx.ptr, tot.ptr, B, T, T40
    rc = lb.stzs_alignment(a, None)
    torch.cuda.synchronize()
    assert rc == want, (rc, want)
    if want != 0:
        return same_bits(idx.t, idx.before) and same_bits(tot.t, tot.before)
    assert idx.untouched() and tot.untouched()
    return idx.rows()[0].view(B, T40).numpy(), tot.rows()[0].numpy()


def _align_rows(T, key):
    """four rows: zeros at the start, in the middle and at the end; a second total; all zeros; no zeros"""
    g = np.random.default_rng(900 + T + key)
    d = g.integers(0, 4, (4, T)).astype(np.int32)
    d[0, 0] = d[0, T // 2] = d[0, T - 1] = 0
    d[1] = g.integers(0, 3, T)
    d[2] = 0
    d[3] = g.integers(1, 5, T)
    return d


@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 4097])
def test_alignment_exact(lib, T):
    """idx and total equal align_ref exactly: zeros anywhere in a row, rows whose totals differ, a row of zeros, and T40
    above every total (-1 tails), equal to one row's total, and below the totals"""
    d = _align_rows(T, 0)
    totals = d.sum(1)
    for T40 in sorted({int(totals.max()) + 3, max(int(totals[0]), 1), max(int(totals[totals > 0].min()) // 2, 1)}):
        want_idx, want_tot = align_ref(d, T40)
        idx, tot = _alignment(lib, d, T40)
        assert np.array_equal(tot, want_tot), (T, T40)
        assert np.array_equal(idx, want_idx), (T, T40, np.argwhere(idx != want_idx)[:4].tolist())


def test_alignment_largest_T_and_refusal(lib):
    """T = 16384, the documented limit (T + 1 scan entries: 65 540 bytes of dynamic LDS), equals align_ref; T = 16385
    returns STZS_ESHAPE and writes nothing"""
    lb, L, dev = lib
    g = np.random.default_rng(16384)
    d = g.integers(0, 3, (2, 16384)).astype(np.int32)
    d[1, -5:] = [0, 2, 0, 0, 1]
    T40 = int(d.sum(1).max()) + 2
    want_idx, want_tot = align_ref(d, T40)
    idx, tot = _alignment(lib, d, T40)
    assert np.array_equal(tot, want_tot) and np.array_equal(idx, want_idx)
    assert _alignment(lib, np.ones((1, 16385), np.int32), 8, want=L.ESHAPE)


# ---- stzs_gather_rows -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cw", [8, 72])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_gather_rows_exact(lib, dtype, Cw):
    """y[b, f, yc0 + c] = x[b, idx[b, f], xc0 + c] in bits, with column offsets on both sides, the first and the last
    source row, and -1 rows all +0; the cells of y outside [yc0, yc0 + C) and behind the rows keep their bits.  x
    carries NaN outside its columns and in a row behind the last."""
    lb, L, dev = lib
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    B, Ts, Td, xc0, yc0 = 2, 9, 14, 8, 16
    ldx, ldy = xc0 + Cw + 8, yc0 + Cw + 8
    g = torch.Generator().manual_seed(Cw)
    x = torch.randn(B, Ts, Cw, generator=g).to(dt)
    xb = torch.full((B, Ts + 1, ldx), NAN, dtype=dt)
    xb[:, :Ts, xc0:xc0 + Cw] = x
    idx = torch.randint(0, Ts, (B, Td), generator=g).int()
    idx[0, 0], idx[0, 1], idx[0, 2], idx[1, Td - 1], idx[1, 0], idx[1, 5] = -1, 0, Ts - 1, -1, Ts - 1, 0
    y = torch.full((B, Td + 2, ldy), SENT, dtype=dt, device=dev)
    before = y.clone()
    xd, idd = xb.to(dev), idx.to(dev)
    a = L.GatherArgs()
    a.x, a.idx, a.y = xd.data_ptr(), idd.data_ptr(), y.data_ptr()
    a.ldx, a.bsx, a.ldy, a.bsy = ldx, (Ts + 1) * ldx, ldy, (Td + 2) * ldy
    a.B, a.Tsrc, a.Tdst, a.C, a.xc0, a.yc0, a.dtype = B, Ts, Td, Cw, xc0, yc0, L.BF16 if dtype == "bf16" else L.F32
    L.check(lb.stzs_gather_rows(a, None), "gather")
    torch.cuda.synchronize()
    want = torch.stack([torch.where(idx[b, :, None] >= 0, x[b, idx[b].clamp_min(0).long()], torch.zeros((), dtype=dt))
                        for b in range(B)])
    assert same_bits(y[:, :Td, yc0:yc0 + Cw].cpu().contiguous(), want)
    may = torch.zeros(y.shape, dtype=torch.bool, device=dev)
    may[:, :Td, yc0:yc0 + Cw] = True
    assert same_bits(y[~may], before[~may])
