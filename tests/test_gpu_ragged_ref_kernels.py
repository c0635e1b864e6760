"""Ragged reference batches at kernel level, straight through the C ABI: the optional length fields of
stzs_stft_logmel and stzs_stft_frames (n_lens in samples, f_lens_out), stzs_log_mel and stzs_pool_rows (lens in rows)
and the new stzs_mask_rows, on SPEC_TINY's framing (n_fft 2048, win 1200, hop 300) and the two batches of the design
note: N = 4500 with lengths [4500, 1025, 2999, 3000] (frames [16, 4, 10, 11]: the shortest legal clip, fewer frames
than L_s, a hop straddled) and N = 39000 with [39000, 38400, 38399, 1025] (frames [131, 129, 128, 4]).

The reference is always the SAME kernel launched alone on that row at N = n_lens[b] (T = lens[b]), compared bit for
bit (torch.equal on the stored values).  Inputs past a row's length are NaN (a read would poison the row), outputs are
over-allocated, non-compact and filled with a guard value that must survive; rows past a length are exact zeros; a
length outside its range behaves as its clamp; a NULL length pointer leaves the launch as it was."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from refops import max_rel

pytestmark = pytest.mark.gpu

BATCHES = {"short": (4500, [4500, 1025, 2999, 3000]), "tile": (39000, [39000, 38400, 38399, 1025])}
GUARD = 7.0


@pytest.fixture(scope="module")
def fe(gpu_device, tiny, tiny_params):
    """library, bindings, device and the front end's constant tables (window, twiddles, filterbank, ranges)"""
    from stzs import _lib as L
    from stzs.weights import PackedModel
    W = PackedModel(tiny, tiny_params, device=gpu_device, precise_frontend=True)
    tabs = dict(win=W.t(W.fe_win), tw=W.t(W.fe_tw), fb=W.t(W.fe_fb), rng=W.t(W.fe_rng))
    return L.load(), L, gpu_device, tiny, tabs


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _poisoned(N, lens, dev):
    """[B, N] noise with NaN at and past every row's length"""
    wav = torch.randn(len(lens), N, generator=torch.Generator().manual_seed(N)) * 0.1
    for b, n in enumerate(lens):
        wav[b, n:] = float("nan")
    return wav.to(dev)


def _clamp(v, lo, hi):
    return [min(max(x, lo), hi) for x in v]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


# ---- stzs_stft_logmel ------------------------------------------------------------------------------------------------

def _stft_logmel(fe, wav, row0, nb, N, dt, lens=None, want_f=False):
    """launch on rows [row0, row0 + nb) of wav at width N -> (y [nb, F, n_mels], whole guarded buffer, f_lens | None)"""
    lib, L, dev, S, tb = fe
    Fr = N // S.hop + 1
    ldy = S.n_mels + 3
    y = torch.full((nb, Fr + 2, ldy), GUARD, dtype=dt, device=dev)
    fl = torch.full((nb + 2,), -1, dtype=torch.int32, device=dev)
    a = L.StftMelArgs()
    a.wav = wav.data_ptr() + row0 * wav.stride(0) * 4
    a.window, a.twiddle, a.fb, a.ranges = (tb[k].data_ptr() for k in ("win", "tw", "fb", "rng"))
    a.y, a.ldw, a.ldy, a.bsy = y.data_ptr(), wav.stride(0), ldy, (Fr + 2) * ldy
    a.B, a.N, a.F, a.n_fft, a.win, a.hop, a.n_mels = nb, N, Fr, S.mel_nfft, S.mel_win, S.hop, S.n_mels
    a.out_dtype = L.BF16 if dt == torch.bfloat16 else L.F32
    if lens is not None:
        a.n_lens = lens.data_ptr()
        if want_f:
            a.f_lens_out = fl.data_ptr() + 4
    L.check(lib.stzs_stft_logmel(C.byref(a), None), "stft_logmel")
    torch.cuda.synchronize()
    assert bool((y[:, Fr:] == GUARD).all()) and bool((y[:, :, S.n_mels:] == GUARD).all()), "guard overwritten"
    assert int(fl[0]) == -1 and int(fl[-1]) == -1
    return y[:, :Fr, :S.n_mels], y, (fl[1:-1] if want_f else None)


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_stft_logmel_lens(fe, name, dt):
    _, _, dev, S, _ = fe
    N, lens = BATCHES[name]
    wav = _poisoned(N, lens, dev)
    y, _, fl = _stft_logmel(fe, wav, 0, len(lens), N, dt, _i32(lens, dev), want_f=True)
    assert fl.tolist() == [n // S.hop + 1 for n in lens]
    for b, n in enumerate(lens):
        Fb = n // S.hop + 1
        solo, _, _ = _stft_logmel(fe, wav, b, 1, n, dt)
        assert torch.equal(_bits(y[b, :Fb]), _bits(solo[0])), f"row {b} (n {n}) differs from its solo launch"
        assert bool((y[b, Fb:] == 0).all()), f"row {b}: frames past its length are not zero"
    assert bool(torch.isfinite(y.float()).all())
    # without f_lens_out: the same rows
    y2, _, _ = _stft_logmel(fe, wav, 0, len(lens), N, dt, _i32(lens, dev))
    assert torch.equal(_bits(y2), _bits(y))


def test_stft_logmel_clamps_and_null(fe):
    """device lengths 0 and N + 7 behave as n_fft / 2 + 1 and N; NULL lengths = the uniform launch = full lengths"""
    _, _, dev, S, _ = fe
    N = 4500
    lo = S.mel_nfft // 2 + 1
    raw = [0, N + 7, 2999, -5]
    eff = _clamp(raw, lo, N)
    wav = _poisoned(N, eff, dev)
    y, _, fl = _stft_logmel(fe, wav, 0, 4, N, torch.float32, _i32(raw, dev), want_f=True)
    want, _, flw = _stft_logmel(fe, wav, 0, 4, N, torch.float32, _i32(eff, dev), want_f=True)
    assert torch.equal(y, want) and torch.equal(fl, flw) and fl.tolist() == [n // S.hop + 1 for n in eff]
    assert bool(torch.isfinite(y).all())
    clean = _poisoned(N, [N] * 4, dev)
    uni, _, _ = _stft_logmel(fe, clean, 0, 4, N, torch.float32)
    full, _, _ = _stft_logmel(fe, clean, 0, 4, N, torch.float32, _i32([N] * 4, dev))
    assert torch.equal(uni, full)
    for b in range(4):
        solo, _, _ = _stft_logmel(fe, clean, b, 1, N, torch.float32)
        assert torch.equal(uni[b], solo[0])


# ---- stzs_stft_frames ------------------------------------------------------------------------------------------------

def _frames(fe, wav, row0, nb, N, lens=None, want_f=False):
    lib, L, dev, S, tb = fe
    Fr = N // S.hop + 1
    ldy = S.mel_win + 8  # (every one of the ldy columns is written: zeros past the window)
    y = torch.full((nb, Fr + 2, ldy), GUARD, dtype=torch.bfloat16, device=dev)
    fl = torch.full((nb + 2,), -1, dtype=torch.int32, device=dev)
    a = L.FramesArgs()
    a.wav, a.window, a.y = wav.data_ptr() + row0 * wav.stride(0) * 4, tb["win"].data_ptr(), y.data_ptr()
    a.ldw, a.ldy, a.bsy = wav.stride(0), ldy, (Fr + 2) * ldy
    a.B, a.N, a.F, a.n_fft, a.win, a.hop = nb, N, Fr, S.mel_nfft, S.mel_win, S.hop
    if lens is not None:
        a.n_lens = lens.data_ptr()
        if want_f:
            a.f_lens_out = fl.data_ptr() + 4
    L.check(lib.stzs_stft_frames(C.byref(a), None), "stft_frames")
    torch.cuda.synchronize()
    assert bool((y[:, Fr:] == GUARD).all()), "guard rows overwritten"
    assert int(fl[0]) == -1 and int(fl[-1]) == -1
    return y[:, :Fr], (fl[1:-1] if want_f else None)


@pytest.mark.parametrize("name", list(BATCHES))
def test_stft_frames_lens(fe, name):
    _, _, dev, S, _ = fe
    N, lens = BATCHES[name]
    wav = _poisoned(N, lens, dev)
    y, fl = _frames(fe, wav, 0, len(lens), N, _i32(lens, dev), want_f=True)
    assert fl.tolist() == [n // S.hop + 1 for n in lens]
    for b, n in enumerate(lens):
        Fb = n // S.hop + 1
        solo, _ = _frames(fe, wav, b, 1, n)
        assert torch.equal(_bits(y[b, :Fb]), _bits(solo[0])), f"row {b} (n {n}) differs from its solo launch"
        assert bool((y[b, Fb:] == 0).all()), f"row {b}: frames past its length are not zero"
    assert bool(torch.isfinite(y.float()).all())


def test_stft_frames_clamps_and_null(fe):
    _, _, dev, S, _ = fe
    N = 4500
    raw = [0, N + 7, 2999, -5]
    eff = _clamp(raw, S.mel_nfft // 2 + 1, N)
    wav = _poisoned(N, eff, dev)
    y, fl = _frames(fe, wav, 0, 4, N, _i32(raw, dev), want_f=True)
    want, flw = _frames(fe, wav, 0, 4, N, _i32(eff, dev), want_f=True)
    assert torch.equal(_bits(y), _bits(want)) and torch.equal(fl, flw)
    assert fl.tolist() == [n // S.hop + 1 for n in eff] and bool(torch.isfinite(y.float()).all())
    clean = _poisoned(N, [N] * 4, dev)
    uni, _ = _frames(fe, clean, 0, 4, N)
    full, _ = _frames(fe, clean, 0, 4, N, _i32([N] * 4, dev))
    assert torch.equal(_bits(uni), _bits(full))
    for b in range(4):
        assert torch.equal(_bits(uni[b]), _bits(_frames(fe, clean, b, 1, N)[0][0]))


# ---- stzs_log_mel ----------------------------------------------------------------------------------------------------

def _log_mel(fe, spec, row0, nb, T, dt, lens=None):
    """spec [B, Tmax, lds] fp32: launch on utterances [row0, row0 + nb), T rows each"""
    lib, L, dev, S, tb = fe
    nbin = S.mel_nfft // 2 + 1
    ldy = S.n_mels + 3
    y = torch.full((nb, T + 2, ldy), GUARD, dtype=dt, device=dev)
    a = L.LogMelArgs()
    a.spec = spec.data_ptr() + row0 * spec.stride(0) * 4
    a.fb, a.ranges, a.y = tb["fb"].data_ptr(), tb["rng"].data_ptr(), y.data_ptr()
    a.lds, a.bss, a.ldy, a.bsy = spec.stride(1), spec.stride(0), ldy, (T + 2) * ldy
    a.B, a.F, a.nbin, a.n_mels = nb, T, nbin, S.n_mels
    a.out_dtype = L.BF16 if dt == torch.bfloat16 else L.F32
    a.lens = lens.data_ptr() if lens is not None else None
    L.check(lib.stzs_log_mel(C.byref(a), None), "log_mel")
    torch.cuda.synchronize()
    assert bool((y[:, T:] == GUARD).all()) and bool((y[:, :, S.n_mels:] == GUARD).all()), "guard overwritten"
    return y[:, :T, :S.n_mels]


def _rows_input(T, lens, width, dev, seed):
    """[B, T, width] fp32 noise, NaN in every row at or past its utterance's length"""
    x = torch.randn(len(lens), T, width, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        x[b, n:] = float("nan")
    return x.to(dev)


@pytest.mark.parametrize("T,lens,raw", [(16, [16, 4, 10, 11], None), (131, [131, 129, 128, 4], None),
                                        (16, [1, 16, 10, 1], [0, 23, 10, -3])], ids=["short", "tile", "clamped"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_log_mel_lens(fe, T, lens, raw, dt):
    _, _, dev, S, _ = fe
    spec = _rows_input(T, lens, 2 * (S.mel_nfft // 2 + 1) + 2, dev, T)
    y = _log_mel(fe, spec, 0, len(lens), T, dt, _i32(raw if raw is not None else lens, dev))
    for b, n in enumerate(lens):
        solo = _log_mel(fe, spec, b, 1, n, dt)
        assert torch.equal(_bits(y[b, :n]), _bits(solo[0])), f"row {b} (len {n}) differs from its solo launch"
        assert bool((y[b, n:] == 0).all())
    assert bool(torch.isfinite(y.float()).all())
    clean = _rows_input(T, [T] * len(lens), spec.shape[2], dev, T)
    assert torch.equal(_bits(_log_mel(fe, clean, 0, len(lens), T, dt)),
                       _bits(_log_mel(fe, clean, 0, len(lens), T, dt, _i32([T] * len(lens), dev))))


# ---- stzs_pool_rows --------------------------------------------------------------------------------------------------

def _pool(fe, x, row0, nb, T, Lr, Cn, dto, lens=None):
    lib, L, dev, _, _ = fe
    ldy = Cn + 5
    y = torch.full((nb, Lr + 1, ldy), GUARD, dtype=dto, device=dev)
    a = L.PoolArgs()
    a.x, a.y = x.data_ptr() + row0 * x.stride(0) * x.element_size(), y.data_ptr()
    a.ldx, a.bsx, a.ldy, a.bsy = x.stride(1), x.stride(0), ldy, (Lr + 1) * ldy
    a.B, a.T, a.L, a.C = nb, T, Lr, Cn
    a.in_dtype = L.BF16 if x.dtype == torch.bfloat16 else L.F32
    a.out_dtype = L.BF16 if dto == torch.bfloat16 else L.F32
    a.lens = lens.data_ptr() if lens is not None else None
    L.check(lib.stzs_pool_rows(C.byref(a), None), "pool_rows")
    torch.cuda.synchronize()
    assert bool((y[:, Lr:] == GUARD).all()) and bool((y[:, :, Cn:] == GUARD).all()), "guard overwritten"
    return y[:, :Lr, :Cn]


@pytest.mark.parametrize("T,lens,raw", [(16, [16, 4, 10, 11], None), (131, [131, 129, 128, 4], None),
                                        (16, [1, 16, 10, 1], [0, 23, 10, -3])], ids=["short", "tile", "clamped"])
@pytest.mark.parametrize("dti", [torch.float32, torch.bfloat16], ids=["in-f32", "in-bf16"])
@pytest.mark.parametrize("dto", [torch.float32, torch.bfloat16], ids=["out-f32", "out-bf16"])
def test_pool_rows_lens(fe, T, lens, raw, dti, dto):
    _, _, dev, S, _ = fe
    Cn, Lr = S.pe_ch, S.L_s  # 32 channels, 8 pooled rows: the 4- and 1-row utterances have fewer rows than L
    x = _rows_input(T, lens, Cn + 8, dev, 100 + T).to(dti)
    y = _pool(fe, x, 0, len(lens), T, Lr, Cn, dto, _i32(raw if raw is not None else lens, dev))
    for b, n in enumerate(lens):
        solo = _pool(fe, x, b, 1, n, Lr, Cn, dto)
        assert torch.equal(_bits(y[b]), _bits(solo[0])), f"row {b} (len {n}) differs from its solo launch"
        if dti == torch.float32 and dto == torch.float32:
            ref = F.adaptive_avg_pool1d(x[b:b + 1, :n, :Cn].cpu().double().transpose(1, 2), Lr).transpose(1, 2)
            assert max_rel(y[b:b + 1].cpu(), ref) < 1e-6
    assert bool(torch.isfinite(y.float()).all())
    clean = _rows_input(T, [T] * len(lens), Cn + 8, dev, 100 + T).to(dti)
    assert torch.equal(_bits(_pool(fe, clean, 0, len(lens), T, Lr, Cn, dto)),
                       _bits(_pool(fe, clean, 0, len(lens), T, Lr, Cn, dto, _i32([T] * len(lens), dev))))


# ---- stzs_mask_rows --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,lens,raw", [(16, [16, 4, 10, 11], None), (131, [131, 129, 128, 4], None),
                                        (16, [1, 16, 10, 1], [0, 23, 10, -3])], ids=["short", "tile", "clamped"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", ["aligned", "odd-ld", "odd-base"])
def test_mask_rows(fe, T, lens, raw, dt, layout):
    """in place on [B, T, C] inside a larger guarded block: rows t >= lens[b] become exact zeros over the C columns,
    everything else keeps its bits -- on the 16-byte store path (aligned) and the element-wide one (a row pitch or a
    base address that is no multiple of 16 bytes)"""
    lib, L, dev, S, _ = fe
    Bn, Cn = len(lens), S.pe_ch
    ld = Cn + (8 if layout != "odd-ld" else 3)
    off = 1 if layout == "odd-base" else 0  # elements
    store = torch.randn(Bn * (T + 2) * ld + 8, generator=torch.Generator().manual_seed(T)).to(dt).to(dev)
    before = store.clone()
    a = L.MaskArgs()
    a.x, a.lens = store.data_ptr() + off * store.element_size(), _i32(raw if raw is not None else lens, dev).data_ptr()
    a.ld, a.bs, a.B, a.T, a.C = ld, (T + 2) * ld, Bn, T, Cn
    a.dtype = L.BF16 if dt == torch.bfloat16 else L.F32
    L.check(lib.stzs_mask_rows(C.byref(a), None), "mask_rows")
    torch.cuda.synchronize()
    want = before.clone()
    blk = want[off:off + Bn * (T + 2) * ld].view(Bn, T + 2, ld)
    for b, n in enumerate(lens):
        blk[b, n:T, :Cn] = 0
    assert torch.equal(_bits(store), _bits(want))
    got = store[off:off + Bn * (T + 2) * ld].view(Bn, T + 2, ld)
    for b, n in enumerate(lens):
        assert bool((got[b, n:T, :Cn] == 0).all())
