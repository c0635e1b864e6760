"""Ragged streaming at kernel level, straight through the C ABI: stzs_istft_stream_args.lens and
.post_off on fp32 random conv_post rows, B = 5, at both accepted geometries (n_fft 20 / hop 5 and 16 / 4).

Every check is bit equality (torch.equal on the stored values).  The references are stzs_istft(lens=...) over the
padded batch and, per row, stzs_istft on that row alone at Tf = Tf_b.  post rows at and past a row's own frame count
are NaN before any call: a read -- or a carried tail row -- would poison the row, so "everything is finite" shows that
they were never read or carried.  The chunk buffers are over-allocated and guarded.

Small case, Tf = 41, lens [41, 2, 17, 16, 40]: with the chunking [16, 25] row 3 (16 frames) ends on the first chunk's
last frame, so its last n_fft / 2 - hop samples come from the next chunk's tail alone; row 2 (17) ends one frame into
the second chunk; row 1 is the minimum of 2; row 4 is one short of full.  [2, 39] puts row 1's last frame on a chunk's
last frame, [8] * 5 + [1] does that for row 3 again (and folds nothing: a 1-frame final chunk), [1] * 41 finalises
every row from tails.  Workgroup-edge case, Tf = 600 (workgroups of 253 frames at both geometries: halo 3), lens
[600, 253, 254, 2, 507]: a row ending on a workgroup's and a chunk's last frame, one frame past it, the minimum, and one
ending inside the third chunk's / second chunk's first workgroup."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 7.0
NAN = float("nan")
B = 5
LDP = 24
GEOMS = [(20, 5), (16, 4)]
SMALL = (41, [41, 2, 17, 16, 40], [[1] * 41, [8] * 5 + [1], [2, 39], [16, 25]])
EDGE = (600, [600, 253, 254, 2, 507], [[253, 253, 94], [300, 300]])


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    # (without the fields a ctypes structure would keep `a.lens = ...` as a plain attribute and launch without it)
    assert [f[0] for f in L.IstftStreamArgs._fields_[-2:]] == ["lens", "post_off"]
    return L.load(), L, gpu_device


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _post(dev, Tf, lens, seed):
    """random rows, NaN at and past each row's own frame count -> device [B, Tf, LDP]"""
    g = torch.Generator().manual_seed(seed)
    post = torch.randn(B, Tf, LDP, generator=g)
    for b, n in enumerate(lens):
        post[b, max(n, 2):] = NAN
    return post.to(dev)


def _istft(lb, geom, post, row0, nb, Tf, lens=None):
    """stzs_istft over rows [row0, row0 + nb) of post at Tf frames"""
    lib_, L, dev = lb
    nfft, hs = geom
    N = (Tf - 1) * hs
    wav = torch.full((nb, N + 8), GUARD, device=dev)
    a = L.IstftArgs()
    a.post, a.wav = post.data_ptr() + row0 * post.stride(0) * 4, wav.data_ptr()
    a.ldp, a.bsp, a.bsw, a.B, a.Tf, a.n_fft, a.hop_s = post.stride(1), post.stride(0), wav.stride(0), nb, Tf, nfft, hs
    if lens is not None:
        a.lens = lens.data_ptr()
    assert lib_.stzs_istft(C.byref(a), None) == 0
    torch.cuda.synchronize()
    assert bool((wav[:, N:] == GUARD).all())
    return wav[:, :N].clone()


def _stream(lb, geom, post, Tf, chunks, lens=None, shift=None):
    """the chunks of stzs_istft_stream concatenated -> [B, (Tf - 1) hop].  shift (a list of B row counts): every chunk's
    frames of row b are handed over shift[b] rows down in a buffer of their own (NaN above them) with post_off = shift
    -- and a negative entry where the shift is 0 (taken as 0)."""
    lib_, L, dev = lb
    nfft, hs = geom
    assert sum(chunks) == Tf
    N = (Tf - 1) * hs
    wav = torch.full((B, N + 8), GUARD, device=dev)
    ldt = 24
    tails = [torch.full((B, 8, ldt), NAN, device=dev) for _ in range(2)]
    off = None if shift is None else _i32([s if s > 0 else -3 for s in shift], dev)
    f0, end = 0, 0
    for i, Fc in enumerate(chunks):
        fin = int(f0 + Fc == Tf)
        n0, n1 = C.c_int64(), C.c_int64()
        halo = lib_.stzs_istft_stream_span(f0, Fc, fin, nfft, hs, C.byref(n0), C.byref(n1))
        assert halo == (nfft + hs - 1) // hs - 1 and n0.value == end
        end = n1.value
        if shift is None:
            src = post[:, f0:f0 + Fc]
            ptr, bsp = post.data_ptr() + f0 * post.stride(1) * 4, post.stride(0)
        else:
            src = torch.full((B, Fc + max(shift), LDP), NAN, device=dev)
            for b, s in enumerate(shift):
                src[b, s:s + Fc] = post[b, f0:f0 + Fc]
            ptr, bsp = src.data_ptr(), src.stride(0)
        a = L.IstftStreamArgs()
        a.post, a.wav = ptr, wav.data_ptr() + n0.value * 4
        a.tail_in = tails[i % 2].data_ptr() if f0 > 0 else None
        a.tail_out = tails[(i + 1) % 2].data_ptr() if not fin else None
        a.ldp, a.bsp, a.bsw, a.ldt = LDP, bsp, wav.stride(0), ldt
        a.B, a.f0, a.Fc, a.final_chunk, a.n_fft, a.hop_s = B, f0, Fc, fin, nfft, hs
        if lens is not None:
            a.lens = lens.data_ptr()
        if off is not None:
            a.post_off = off.data_ptr()
        rc = lib_.stzs_istft_stream(C.byref(a), None)
        assert rc == 0, (rc, i)
        torch.cuda.synchronize()  # (src lives until the launch is done)
        f0 += Fc
    assert end == N and bool((wav[:, N:] == GUARD).all()), "a wav guard was overwritten"
    return wav[:, :N].clone()


_REF = {}


def _refs(lb, geom, case):
    """(post, the padded batch's stzs_istft(lens), [each row's own stzs_istft at Tf_b]) -- computed once per case"""
    Tf, lens, _ = case
    key = (geom, Tf)
    if key not in _REF:
        dev = lb[2]
        post = _post(dev, Tf, lens, 100 + Tf + geom[0])
        whole = _istft(lb, geom, post, 0, B, Tf, _i32(lens, dev))
        solo = [_istft(lb, geom, post, b, 1, max(n, 2))[0] for b, n in enumerate(lens)]
        _REF[key] = (post, whole, solo)
    return _REF[key]


def _check(lb, geom, case, chunks, shift=None):
    Tf, lens, _ = case
    hs = geom[1]
    post, whole, solo = _refs(lb, geom, case)
    got = _stream(lb, geom, post, Tf, chunks, _i32(lens, lb[2]), shift)
    assert bool(torch.isfinite(got).all()), "a frame past a row's own count was read or carried"
    assert torch.equal(got, whole), "the concatenated chunks differ from stzs_istft(lens)"
    for b, n in enumerate(lens):
        E = (max(n, 2) - 1) * hs
        assert solo[b].shape == (E,) and bool(torch.isfinite(solo[b]).all())
        assert torch.equal(got[b, :E], solo[b]), f"row {b} ({n} frames) differs from the row alone at Tf = {n}"
        assert bool((got[b, E:] == 0).all()), f"row {b}: samples at and past its own end are not exact zeros"


@pytest.mark.parametrize("geom", GEOMS, ids=["20_5", "16_4"])
@pytest.mark.parametrize("chunks", SMALL[2], ids=["1x41", "8x5+1", "2+39", "16+25"])
def test_small_rows_match_solo(lib, geom, chunks):
    _check(lib, geom, SMALL, chunks)


@pytest.mark.parametrize("geom", GEOMS, ids=["20_5", "16_4"])
@pytest.mark.parametrize("chunks", EDGE[2], ids=["253+253+94", "300+300"])
def test_workgroup_edge_rows_match_solo(lib, geom, chunks):
    _check(lib, geom, EDGE, chunks)


@pytest.mark.parametrize("geom", GEOMS, ids=["20_5", "16_4"])
def test_post_off_moves_the_rows_not_the_result(lib, geom):
    """each row's chunk frames handed over at a row offset of its own (0 given as a negative entry): same bits"""
    _check(lib, geom, SMALL, [16, 25], shift=[3, 0, 1, 7, 2])
    _check(lib, geom, SMALL, [8] * 5 + [1], shift=[0, 5, 0, 2, 9])
    _check(lib, geom, EDGE, [253, 253, 94], shift=[1, 0, 300, 2, 5])


@pytest.mark.parametrize("geom", GEOMS, ids=["20_5", "16_4"])
def test_full_lengths_equal_null(lib, geom):
    """lens = [Tf] * B is the launch without lens, bit for bit; so is post_off = 0"""
    dev = lib[2]
    for Tf, chunks in ((41, [16, 25]), (41, [1] * 41), (600, [253, 253, 94])):
        post = torch.randn(B, Tf, LDP, generator=torch.Generator().manual_seed(Tf + geom[1])).to(dev)
        plain = _stream(lib, geom, post, Tf, chunks)
        assert torch.equal(plain, _istft(lib, geom, post, 0, B, Tf))
        assert torch.equal(_stream(lib, geom, post, Tf, chunks, _i32([Tf] * B, dev)), plain)
        assert torch.equal(_stream(lib, geom, post, Tf, chunks, _i32([Tf + 9] * B, dev), shift=[0] * B), plain)


def test_tail_rows_past_the_end_are_zeros(lib):
    """the carried tail of a ragged launch: the rows of frames >= Tf_b are stored as zeros, the others are the raw rows"""
    lib_, L, dev = lib
    nfft, hs, Tf, lens = 20, 5, 41, [41, 2, 17, 16, 40]
    post = _post(dev, Tf, lens, 9)
    tail = torch.full((B, 8, 24), NAN, device=dev)
    wav = torch.full((B, 16 * hs + 8), GUARD, device=dev)
    a = L.IstftStreamArgs()
    a.post, a.wav, a.tail_out = post.data_ptr(), wav.data_ptr(), tail.data_ptr()
    a.ldp, a.bsp, a.bsw, a.ldt = LDP, post.stride(0), wav.stride(0), 24
    a.B, a.f0, a.Fc, a.final_chunk, a.n_fft, a.hop_s = B, 0, 18, 0, nfft, hs
    a.lens = _i32(lens, dev).data_ptr()
    assert lib_.stzs_istft_stream(C.byref(a), None) == 0
    torch.cuda.synchronize()
    for b, n in enumerate(lens):  # the tail is [B][halo = 3][ldt = 24]: frames 15, 16, 17 of row b
        rows = tail.flatten()[b * 3 * 24:(b + 1) * 3 * 24].reshape(3, 24)[:, :nfft + 2]
        for i, f in enumerate((15, 16, 17)):
            want = post[b, f, :nfft + 2] if f < n else torch.zeros(nfft + 2, device=dev)
            assert torch.equal(rows[i], want), (b, f)
