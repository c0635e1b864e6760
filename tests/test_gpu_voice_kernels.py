"""stzs_voice_prompt (csrc/voice.hip) through the raw entry point on synthetic codebooks, no engine.
Everything is compared for equality: the mix against tests/refops_voice.py mix_ref (numpy float32, the header's order),
the indices and dequantised rows against the oracle's product VQ of that, the gather form against the mix form and
against stzs_code_quantize.  Shapes: (B, L) = (1, 8) a partial 64-row tile, (8, 8) exactly one, (9, 8) one and a
partial one, (1, 50) / (3, 50) the v0 row count; K = 256 and K = 5 (a K the four scan waves do not divide: ranges of 2,
2, 1 and 0 entries); dg over every width the kernel has; Kmax 1, 2, 3 and 8 with a different source count per row."""
import ctypes as C

import numpy as np
import pytest
import torch

from refops_voice import mix_ref, vq_ref

pytestmark = pytest.mark.gpu

G = 3  # groups: the code width is G * dg
V = 6  # bank rows: voices 0 .. 4 and a row of NaN at V - 1 that no counted source names
SHAPES = [(1, 8), (8, 8), (9, 8), (1, 50), (3, 50)]


def _launch(dev, zbank, ibank, cb, src, w, cnt, B, L, gather=0, zmix=True):
    """one stzs_voice_prompt launch on host arrays -> (idx, y, zmix | None) host tensors; the outputs start as
    poison (-7 / NaN) so that an element the launch leaves unwritten shows"""
    from stzs import _lib
    lib = _lib.load()
    Gn, K, dg = cb.shape
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev)
    zb, cbd = t(zbank, torch.float32), t(cb, torch.float32)
    ib = None if ibank is None else t(ibank, torch.int32)
    sd, wd, cd = t(src, torch.int32), t(w, torch.float32), t(cnt, torch.int32)
    idx = torch.full((B, L, Gn), -7, dtype=torch.int32, device=dev)
    y = torch.full((B, L, Gn * dg), float("nan"), device=dev)
    zm = torch.full((B, L, Gn * dg), float("nan"), device=dev) if zmix else None
    a = _lib.VoiceArgs()
    a.zbank, a.ibank, a.codebook = zb.data_ptr(), (ib.data_ptr() if ib is not None else None), cbd.data_ptr()
    a.src, a.w, a.cnt, a.idx, a.y = sd.data_ptr(), wd.data_ptr(), cd.data_ptr(), idx.data_ptr(), y.data_ptr()
    a.zmix = zm.data_ptr() if zmix else None
    a.ldz, a.ldib, a.ldi, a.ldy, a.ldm = Gn * dg, Gn, Gn, Gn * dg, Gn * dg
    a.V, a.L, a.B, a.Kmax, a.G, a.K, a.dg, a.gather = zb.shape[0], L, B, sd.shape[1], Gn, K, dg, gather
    _lib.check(lib.stzs_voice_prompt(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "voice_prompt")
    torch.cuda.synchronize(dev)
    return idx.cpu(), y.cpu(), (zm.cpu() if zmix else None)


def _quantize(dev, cb, z):
    """stzs_code_quantize on rows z [R, C] -> (idx [R, G], y [R, C])"""
    from stzs import _lib
    lib = _lib.load()
    Gn, K, dg = cb.shape
    x = torch.as_tensor(np.ascontiguousarray(z)).to(dev)
    cbd = torch.as_tensor(cb).to(dev)
    R = x.shape[0]
    idx = torch.empty(R, Gn, dtype=torch.int32, device=dev)
    y = torch.empty(R, Gn * dg, device=dev)
    a = _lib.VqArgs()
    a.x, a.codebook, a.idx, a.y = x.data_ptr(), cbd.data_ptr(), idx.data_ptr(), y.data_ptr()
    a.ldx, a.ldi, a.ldy, a.R, a.G, a.K, a.dg, a.lookup = Gn * dg, Gn, Gn * dg, R, Gn, K, dg, 0
    _lib.check(lib.stzs_code_quantize(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "vq")
    torch.cuda.synchronize(dev)
    return idx.cpu(), y.cpu()


def _case(dg, K, B, L, Kmax, seed=0):
    """codebook [G, K, dg], bank [V, L, C] (row V - 1 NaN), src / w / cnt with cnt[b] = 1 + (b + Kmax - 1) % Kmax (row 0
    uses all Kmax sources); every entry k >= cnt[b] names the NaN row and carries a NaN weight"""
    rng = np.random.default_rng(1000 * dg + 10 * K + B + L + Kmax + seed)
    cb = (rng.standard_normal((G, K, dg)) * 0.2).astype(np.float32)
    zb = (rng.standard_normal((V, L, G * dg)) * 0.2).astype(np.float32)
    zb[V - 1] = np.nan
    cnt = np.array([1 + (b + Kmax - 1) % Kmax for b in range(B)], dtype=np.int32)
    src = rng.integers(0, V - 1, (B, Kmax)).astype(np.int32)
    w = rng.random((B, Kmax)).astype(np.float32) + np.float32(0.05)
    for b in range(B):
        src[b, cnt[b]:] = V - 1
        w[b, cnt[b]:] = np.nan
    return cb, zb, src, w, cnt


def _same(a, b):
    return a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


@pytest.mark.parametrize("Kmax", [1, 2, 3, 8])
@pytest.mark.parametrize("B,L", SHAPES)
@pytest.mark.parametrize("K", [256, 5])
@pytest.mark.parametrize("dg", [4, 8, 16])
def test_mix_form_matches_reference(gpu_device, dg, K, B, L, Kmax):
    cb, zb, src, w, cnt = _case(dg, K, B, L, Kmax)
    idx, y, zm = _launch(gpu_device, zb, None, cb, src, w, cnt, B, L)
    want_z = mix_ref(zb, src, w, cnt)
    assert np.isfinite(want_z).all()  # (the reference never read the NaN row either)
    assert bool(torch.isfinite(zm).all()) and bool(torch.isfinite(y).all())  # entries k >= cnt[b] were not read
    assert zm.numpy().tobytes() == want_z.tobytes()
    want_idx, want_q = vq_ref(cb, want_z)
    assert torch.equal(idx, want_idx)
    assert _same(y, want_q)
    # the unread entries changed to other (valid) values: nothing changes
    src2, w2 = src.copy(), w.copy()
    for b in range(B):
        src2[b, cnt[b]:], w2[b, cnt[b]:] = 0, 1.0
    idx2, y2, zm2 = _launch(gpu_device, zb, None, cb, src2, w2, cnt, B, L)
    assert torch.equal(idx2, idx) and _same(y2, y) and _same(zm2, zm)
    # zmix NULL: idx and y are the same
    idx3, y3, none = _launch(gpu_device, zb, None, cb, src, w, cnt, B, L, zmix=False)
    assert none is None and torch.equal(idx3, idx) and _same(y3, y)
    # row independence: row b of the batch is the row run alone
    for b in sorted({0, B // 2, B - 1}):
        i1, y1, z1 = _launch(gpu_device, zb, None, cb, src[b:b + 1], w[b:b + 1], cnt[b:b + 1], 1, L)
        assert torch.equal(i1[0], idx[b]) and _same(y1[0], y[b]) and _same(z1[0], zm[b]), b


@pytest.mark.parametrize("B,L", SHAPES)
@pytest.mark.parametrize("K", [256, 5])
@pytest.mark.parametrize("dg", [4, 8, 16])
def test_gather_form_is_the_mix_form_at_weight_one(gpu_device, dg, K, B, L):
    """gather == mix at cnt = 1, w = 1 == stzs_code_quantize of the bank rows, on a bank whose stored indices are the
    mix form's own"""
    cb, zb, _, _, _ = _case(dg, K, B, L, 1)
    zb = zb[:V - 1]  # (no NaN row: every voice is named here)
    Vn = V - 1
    ids = np.arange(Vn, dtype=np.int32).reshape(Vn, 1)
    one, c1 = np.ones((Vn, 1), np.float32), np.ones(Vn, np.int32)
    ibank, qbank, zback = _launch(gpu_device, zb, None, cb, ids, one, c1, Vn, L)  # enrolment: voice v alone
    assert zback.numpy().tobytes() == zb.tobytes()  # 1.0f * z is z
    src = np.array([[(3 * b + 1) % Vn] for b in range(B)], dtype=np.int32)
    wB, cB = np.ones((B, 1), np.float32), np.ones(B, np.int32)
    mi, my, mz = _launch(gpu_device, zb, None, cb, src, wB, cB, B, L)
    # (the gather form reads neither w nor cnt: poison there must not matter)
    gi, gy, gz = _launch(gpu_device, zb, ibank.numpy(), cb, src, np.full((B, 1), np.nan, np.float32),
                         np.full(B, 99, np.int32), B, L, gather=1)
    assert torch.equal(gi, mi) and _same(gy, my) and _same(gz, mz)
    gi2, gy2, none = _launch(gpu_device, zb, ibank.numpy(), cb, src, wB, cB, B, L, gather=1, zmix=False)
    assert none is None and torch.equal(gi2, gi) and _same(gy2, gy)
    rows = zb[src[:, 0]].reshape(B * L, G * dg)
    qi, qy = _quantize(gpu_device, cb, rows)
    assert torch.equal(qi.reshape(B, L, G), gi) and _same(qy.reshape(B, L, G * dg), gy)
    want_idx, want_q = vq_ref(cb, zb[src[:, 0]])
    assert torch.equal(gi, want_idx) and _same(gy, want_q)


@pytest.mark.parametrize("K", [256, 5])
@pytest.mark.parametrize("dg", [4, 8, 16])
def test_ties_take_the_first_index(gpu_device, dg, K):
    """duplicated codebook rows -- inside one wave's range and across two -- and bank rows that ARE those entries
    (distance exactly 0 to both copies): the first index wins; a voice blended with itself at (0.5, 0.5) keeps its
    stored indices"""
    L, B = 8, 2
    cb, zb, _, _, _ = _case(dg, K, B, L, 2, seed=7)
    zb = zb[:V - 1]
    lo, near, far = 1, 3, (200 if K > 5 else 4)  # K = 256: ranges of 64; K = 5: ranges [0, 2) [2, 4) [4, 5)
    cb[:, near] = cb[:, lo]
    cb[:, far] = cb[:, lo]
    cb[:, 0] = cb[:, lo] + np.float32(1.0)  # (index 0 is no winner by default)
    for g in range(G):
        zb[0, :, g * dg:(g + 1) * dg] = cb[g, lo]
    ids = np.arange(V - 1, dtype=np.int32).reshape(-1, 1)
    ibank, _, _ = _launch(gpu_device, zb, None, cb, ids, np.ones((V - 1, 1), np.float32), np.ones(V - 1, np.int32),
                          V - 1, L)
    assert bool((ibank[0] == lo).all())
    want_idx, _ = vq_ref(cb, zb)
    assert torch.equal(ibank, want_idx)
    src = np.array([[0, 0], [3, 3]], dtype=np.int32)
    half = np.full((2, 2), 0.5, np.float32)
    idx, y, zm = _launch(gpu_device, zb, None, cb, src, half, np.array([2, 2], np.int32), 2, L)
    assert zm.numpy().tobytes() == zb[[0, 3]].tobytes()
    assert torch.equal(idx, ibank[[0, 3]])


@pytest.mark.parametrize("dg", [4, 8, 16])
def test_device_values_are_clamped(gpu_device, dg):
    """ids of -3 and V + 7 in the device array behave as 0 and V - 1, cnt of 0 and Kmax + 2 as 1 and Kmax (both forms)"""
    K, B, L, Kmax = 256, 4, 8, 3
    cb, zb, src, w, _ = _case(dg, K, B, L, Kmax)
    zb = zb[:V - 1]
    Vn = V - 1
    src = np.array([[-3, 1, 2], [Vn + 7, 0, 1], [2, -3, Vn + 7], [1, 2, 3]], dtype=np.int32)
    ok = np.array([[0, 1, 2], [Vn - 1, 0, 1], [2, 0, Vn - 1], [1, 2, 3]], dtype=np.int32)
    w = np.abs(w) + np.float32(0.1)
    w[~np.isfinite(w)] = np.float32(0.5)
    cnt = np.array([0, Kmax + 2, 2, -5], dtype=np.int32)
    okc = np.array([1, Kmax, 2, 1], dtype=np.int32)
    got = _launch(gpu_device, zb, None, cb, src, w, cnt, B, L)
    want = _launch(gpu_device, zb, None, cb, ok, w, okc, B, L)
    assert torch.equal(got[0], want[0]) and _same(got[1], want[1]) and _same(got[2], want[2])
    assert got[2].numpy().tobytes() == mix_ref(zb, src, w, cnt).tobytes()  # (the reference clamps the same way)
    ids = np.arange(Vn, dtype=np.int32).reshape(-1, 1)
    ibank, _, _ = _launch(gpu_device, zb, None, cb, ids, np.ones((Vn, 1), np.float32), np.ones(Vn, np.int32), Vn, L)
    g1 = _launch(gpu_device, zb, ibank.numpy(), cb, src[:, :1], w[:, :1], cnt, B, L, gather=1)
    g2 = _launch(gpu_device, zb, ibank.numpy(), cb, ok[:, :1], w[:, :1], okc, B, L, gather=1)
    assert torch.equal(g1[0], g2[0]) and _same(g1[1], g2[1]) and _same(g1[2], g2[2])
    assert torch.equal(g1[0], ibank[ok[:, 0]])
