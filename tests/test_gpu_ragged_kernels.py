"""Ragged text batches at kernel level (DESIGN.md "Ragged text batches"), straight through the C ABI: the optional
length arguments of stzs_lstm / stzs_lstm_pair (lens), stzs_attention (lk_rows), stzs_row_layernorm (lens, T),
stzs_embed_lens, stzs_predictor_prep (lens), stzs_durations (lens) and stzs_copy2d (dst_row_off).

The reference is always the SAME kernel launched alone on that row at its own length, compared bit for bit
(torch.equal on the stored values) -- the project's standard for row and batch invariance -- and what lies past a
row's length is exactly zero where the interface says so.  A NULL length pointer must leave the call as it was."""
import math

import pytest
import torch
import torch.nn.functional as F

from refops import same_bits, ulp_diff

pytestmark = pytest.mark.gpu

B3, T6, LENS3 = 3, 6, [6, 1, 4]  # the row kernels' batch: a full row, a one-token row, a row in between


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ---- stzs_lstm / stzs_lstm_pair ------------------------------------------------------------------------------------

def _lstm_weights(H, precise, seed, dev):
    """random W_hh of both directions as the kernel's B fragments (stzs/weights.py lstm_frags; precise: hi then lo)"""
    from stzs.weights import lstm_frags, split_bf16
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / math.sqrt(H)
    w = [(torch.rand(4 * H, H, generator=g) * 2 - 1) * k for _ in range(2)]
    if precise:
        parts = [split_bf16(v) for v in w]
        fr = torch.stack([torch.stack([lstm_frags(parts[d][h].float()) for d in range(2)], 0) for h in range(2)], 0)
    else:
        fr = torch.stack([lstm_frags(v) for v in w], 0)
    return fr.to(torch.bfloat16).contiguous().to(dev)


class _Lstm:
    """one recurrence's launch state: gates gx [B, T, 8H] fp32, output y, its own exchange workspace and sync words"""

    def __init__(self, lb, L, dev, whh, gx, H, precise, lens=None):
        self.B, self.T = gx.shape[:2]
        self.gx = gx.contiguous().to(dev)
        self.y = torch.full((self.B, self.T, 2 * H), 7.0, dtype=torch.float32 if precise else torch.bfloat16,
                            device=dev)
        self.xchg = torch.zeros(max(lb.stzs_lstm_workspace(self.B, H, 2), 16), dtype=torch.uint8, device=dev)
        self.sync = torch.zeros(4096, dtype=torch.uint8, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lens = None if lens is None else _i32(lens, dev)
        a = self.a = L.LstmArgs()
        a.gx, a.whhT, a.y, a.xchg, a.sync = (t.data_ptr() for t in (self.gx, whh, self.y, self.xchg, self.sync))
        a.ldg, a.bsg, a.ldy, a.bsy = 8 * H, self.T * 8 * H, 2 * H, self.T * 2 * H
        a.B, a.T, a.H, a.ndir, a.precise = self.B, self.T, H, 2, precise
        a.status = self.status.data_ptr()
        a.lens = self.lens.data_ptr() if self.lens is not None else None

    def done(self):
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0, "LSTM exchange timed out"
        return self.y.cpu()


def _lstm_run(lb, L, dev, whh, gx, H, precise, lens=None):
    r = _Lstm(lb, L, dev, whh, gx, H, precise, lens)
    L.check(lb.stzs_lstm(r.a, None), "lstm")
    return r.done()


def _check_rows(y, lens, solo):
    """y [B, T, 2H] of a ragged launch: row b's first lens[b] steps are the solo launch's bits, the rest exact zeros"""
    for b, n in enumerate(lens):
        assert torch.equal(y[b, :n], solo(b, n)[0]), f"row {b} (len {n}) differs from its solo launch"
        assert bool((y[b, n:] == 0).all()), f"row {b}: y past its length is not zero"


@pytest.mark.parametrize("lens", [[4, 7], [9, 1, 5]], ids=["tagged-B2", "counter-B3"])
@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("H", [32, 64])
def test_lstm_lens(lib, H, precise, lens):
    """B = 2 (the tagged batch <= 2 cell map; split-operand mode always exchanges through the counters) and B = 3
    (the counter form; lengths 1 and T included): row b at t < lens[b] equals a B = 1, T = lens[b] launch on
    gx[b, :lens[b]], y[b, t >= lens[b]] == 0, the status word stays 0, and lens = NULL is the unchanged call."""
    lb, L, dev = lib
    Bn, T = len(lens), max(lens)
    whh = _lstm_weights(H, precise, 11 + H, dev)
    gx = torch.randn(Bn, T, 8 * H, generator=torch.Generator().manual_seed(100 * H + Bn + precise))
    y = _lstm_run(lb, L, dev, whh, gx, H, precise, lens)
    assert bool(torch.isfinite(y.float()).all())
    _check_rows(y, lens, lambda b, n: _lstm_run(lb, L, dev, whh, gx[b:b + 1, :n], H, precise))
    # NULL lens == full lengths == the call without the field (the struct's zero default)
    y_null = _lstm_run(lb, L, dev, whh, gx, H, precise)
    y_full = _lstm_run(lb, L, dev, whh, gx, H, precise, [T] * Bn)
    assert torch.equal(y_null, y_full)
    for b in range(Bn):
        assert torch.equal(y_null[b:b + 1], _lstm_run(lb, L, dev, whh, gx[b:b + 1], H, precise)), b


def test_lstm_pair_lens(lib):
    """stzs_lstm_pair: two recurrences of different T side by side, each with its OWN lens (and one with none): each
    is the bits of its own stzs_lstm call with that lens."""
    lb, L, dev = lib
    H = 64
    whh = _lstm_weights(H, 0, 5, dev)
    g = torch.Generator().manual_seed(9)
    gxa, gxb = torch.randn(3, 9, 8 * H, generator=g), torch.randn(3, 6, 8 * H, generator=g)
    la, lb_ = [9, 1, 5], [2, 6, 3]
    ra, rb = _lstm_run(lb, L, dev, whh, gxa, H, 0, la), _lstm_run(lb, L, dev, whh, gxb, H, 0, lb_)
    rb_none = _lstm_run(lb, L, dev, whh, gxb, H, 0)
    for second, want in ((lb_, rb), (None, rb_none)):
        pa, pb = _Lstm(lb, L, dev, whh, gxa, H, 0, la), _Lstm(lb, L, dev, whh, gxb, H, 0, second)
        L.check(lb.stzs_lstm_pair(pa.a, pb.a, None), "lstm_pair")
        assert torch.equal(pa.done(), ra) and torch.equal(pb.done(), want)


# ---- stzs_attention ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["cross", "sep"])
@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("dh", [32, 64])
def test_attention_lk_rows(lib, dh, precise, layout):
    """Lq = 50, Lk = 173, lk_rows = [173, 9, 64, 65] (all keys, part of a chunk, exactly one chunk, one key into the
    second): k / v rows at or beyond lk_rows[r] hold NaN, row r equals an R = 1, Lk = lk_rows[r] launch on its first
    lk_rows[r] keys, and the output is finite."""
    lb, L, dev = lib
    heads, Lq, Lk = 2, 50, 173
    lk = [173, 9, 64, 65]
    R, D = len(lk), heads * dh
    dt, es = (torch.float32, 4) if precise else (torch.bfloat16, 2)
    g = torch.Generator().manual_seed(1000 * dh + precise)
    q = torch.randn(R, Lq, D, generator=g).to(dt)
    kv = torch.randn(R, Lk, 2 * D, generator=g).to(dt)
    for r, n in enumerate(lk):
        kv[r, n:] = float("nan")

    def launch(qr, kvr, Lkk, lk_rows):
        rows = qr.shape[0]
        qd = qr.contiguous().to(dev)
        a = L.AttnArgs()
        if layout == "cross":  # k | v column slices of one buffer
            kd = vd = kvr.contiguous().to(dev)
            a.k, a.v, a.ldk, a.ldv = kd.data_ptr(), kd.data_ptr() + D * es, 2 * D, 2 * D
        else:
            kd, vd = kvr[..., :D].contiguous().to(dev), kvr[..., D:].contiguous().to(dev)
            a.k, a.v, a.ldk, a.ldv = kd.data_ptr(), vd.data_ptr(), D, D
        a.bsk, a.bsv = kvr.shape[1] * a.ldk, kvr.shape[1] * a.ldv
        o = torch.full((rows, Lq, D), -777.0, dtype=dt, device=dev)
        a.q, a.o, a.ldq, a.ldo, a.bsq, a.bso = qd.data_ptr(), o.data_ptr(), D, D, Lq * D, Lq * D
        a.R, a.Lq, a.Lk, a.heads, a.dh, a.precise = rows, Lq, Lkk, heads, dh, precise
        lkd = None if lk_rows is None else _i32(lk_rows, dev)
        a.lk_rows = lkd.data_ptr() if lkd is not None else None
        L.check(lb.stzs_attention(a, None), "attention")
        torch.cuda.synchronize()
        return o.cpu()

    o = launch(q, kv, Lk, lk)
    assert bool(torch.isfinite(o.float()).all())
    for r, n in enumerate(lk):
        solo = launch(q[r:r + 1], kv[r:r + 1, :n], n, None)
        assert same_bits(o[r:r + 1], solo), f"row {r} (lk {n})"


# ---- stzs_row_layernorm --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_row_layernorm_lens(lib, dtype):
    """B = 3, T = 6, C = 64, lens [6, 1, 4], affine LayerNorm + LeakyReLU 0.2 (the text CNN's): kept rows have the
    bits of the launch without the mask, masked rows are exact zeros."""
    lb, L, dev = lib
    C = 64
    dt, dti = (torch.bfloat16, L.BF16) if dtype == "bf16" else (torch.float32, L.F32)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B3 * T6, C, generator=g) * 2 + 0.5).to(dt).to(dev)
    G, Bt = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    lens = _i32(LENS3, dev)

    def run(masked):
        y = torch.full((B3 * T6, C), 5.0, dtype=dt, device=dev)
        a = L.RowLNArgs()
        a.x, a.y, a.G, a.Bt = x.data_ptr(), y.data_ptr(), G.data_ptr(), Bt.data_ptr()
        a.ldx, a.ldy, a.R, a.C, a.gdiv, a.in_dtype, a.out_dtype = C, C, B3 * T6, C, 1, dti, dti
        a.act, a.slope, a.eps = L.ACT_LEAKY, 0.2, 1e-5
        if masked:
            a.lens, a.T = lens.data_ptr(), T6
        L.check(lb.stzs_row_layernorm(a, None), "rowln")
        torch.cuda.synchronize()
        return y.cpu().view(B3, T6, C)

    full, got = run(False), run(True)
    assert bool((full != 0).any(-1).all())  # (an unmasked row is never all zeros: the mask is what zeroes)
    for b, n in enumerate(LENS3):
        assert same_bits(got[b, :n].contiguous(), full[b, :n].contiguous()), b
        assert bool((got[b, n:] == 0).all()), b


# ---- stzs_embed_lens -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_embed_lens(lib, dtype):
    """kept rows equal stzs_embed / stzs_embed_f32 on that row alone at its own length, the rest are zeros; the
    tokens of the padding are out of the table's range (they must not be read as indices)."""
    lb, L, dev = lib
    nsym, D, ldy = 20, 40, 48
    dt, dti = (torch.bfloat16, L.BF16) if dtype == "bf16" else (torch.float32, L.F32)
    g = torch.Generator().manual_seed(4)
    emb = torch.randn(nsym, D, generator=g).to(dev)
    tok = torch.randint(0, nsym, (B3, T6), generator=g, dtype=torch.int32)
    for b, n in enumerate(LENS3):
        tok[b, n:] = 1 << 30
    tokd, lens = tok.to(dev), _i32(LENS3, dev)
    y = torch.full((B3, T6, ldy), 5.0, dtype=dt, device=dev)
    L.check(lb.stzs_embed_lens(tokd.data_ptr(), emb.data_ptr(), y.data_ptr(), lens.data_ptr(), B3, T6, D, ldy, dti,
                               None), "embed_lens")
    torch.cuda.synchronize()
    assert bool((y[:, :, D:] == 5.0).all())  # the row pitch past D is not written
    solo_fn = lb.stzs_embed if dtype == "bf16" else lb.stzs_embed_f32
    for b, n in enumerate(LENS3):
        tb = tok[b:b + 1, :n].contiguous().to(dev)
        ys = torch.full((1, n, ldy), 5.0, dtype=dt, device=dev)
        L.check(solo_fn(tb.data_ptr(), emb.data_ptr(), ys.data_ptr(), 1, n, D, ldy, None), "embed")
        torch.cuda.synchronize()
        assert same_bits(y[b, :n, :D].cpu().contiguous(), ys[0, :, :D].cpu().contiguous()), b
        assert bool((y[b, n:, :D] == 0).all()), b


# ---- stzs_predictor_prep -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f32", [0, 1])
def test_predictor_prep_lens(lib, f32):
    """row b's first lens[b] rows equal the solo launch at T = lens[b] (the ratio is L / lens[b]) and torch's
    F.interpolate(size = lens[b]) at tests/test_gpu_glue.py's tolerance for stzs_predictor_prep (fp32: 4 * 2^-24
    max|codes|, the FMA contraction of the two-tap sum; bf16: one ulp of the rounded value); pad rows are zeros
    over the text and the style columns."""
    lb, L, dev = lib
    Lc, Ch, Cs = 8, 64, 32
    dt = torch.float32 if f32 else torch.bfloat16
    g = torch.Generator().manual_seed(6 + f32)
    codes = torch.randn(B3, Lc, Cs, generator=g)
    h = torch.randn(B3, T6, Ch, generator=g).to(dt)

    def run(cd, hh, lens):
        Bn, T = hh.shape[:2]
        cdd, hd = cd.contiguous().to(dev), hh.contiguous().to(dev)
        y = torch.full((Bn, T, Ch + Cs), 5.0, dtype=dt, device=dev)
        ld = None if lens is None else _i32(lens, dev)
        a = L.PrPrepArgs()
        a.codes, a.h, a.y = cdd.data_ptr(), hd.data_ptr(), y.data_ptr()
        a.ldc, a.bsc, a.ldh, a.bsh, a.ldy, a.bsy = Cs, Lc * Cs, Ch, T * Ch, Ch + Cs, T * (Ch + Cs)
        a.B, a.L, a.T, a.c0, a.Cs, a.Ch, a.yc0, a.f32 = Bn, Lc, T, 0, Cs, Ch, Ch, f32
        a.lens = ld.data_ptr() if ld is not None else None
        L.check(lb.stzs_predictor_prep(a, None), "prprep")
        torch.cuda.synchronize()
        return y.cpu()

    got = run(codes, h, LENS3)
    for b, n in enumerate(LENS3):
        solo = run(codes[b:b + 1], h[b:b + 1, :n], None)
        assert same_bits(got[b, :n].contiguous(), solo[0].contiguous()), b
        assert bool((got[b, n:] == 0).all()), b
        t32 = F.interpolate(codes[b:b + 1].transpose(1, 2), size=n, mode="linear", align_corners=False)[0].t()
        z = got[b, :n, Ch:].contiguous()
        if f32:
            d, tol = (z - t32).abs().max().item(), 4 * 2.0 ** -24 * codes.abs().max().item()
            print(f"prprep lens row {b} (len {n}): max |y - torch fp32| = {d:.3e} (bound {tol:.3e})")
            assert d <= tol
        else:
            assert ulp_diff(z, t32.to(torch.bfloat16).contiguous()) <= 1


# ---- stzs_durations ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("forced", [False, True])
def test_durations_lens(lib, forced):
    """dur and dsum of t < lens[b] equal the solo launch, both are 0 past it -- a forced duration there too"""
    lb, L, dev = lib
    nb = 8
    g = torch.Generator().manual_seed(8)
    logits = torch.randn(B3, T6, nb, generator=g) * 2
    ov = torch.randint(1, 9, (B3, T6), generator=g, dtype=torch.int32) if forced else None

    def run(lg, o, lens):
        Bn, T = lg.shape[:2]
        lgd = lg.contiguous().to(dev)
        od = None if o is None else o.contiguous().to(dev)
        ld = None if lens is None else _i32(lens, dev)
        dur = torch.full((Bn, T), -5, dtype=torch.int32, device=dev)
        ds = torch.full((Bn, T), -5.0, device=dev)
        a = L.DurArgs()
        a.logits, a.dur, a.dsum = lgd.data_ptr(), dur.data_ptr(), ds.data_ptr()
        a.override_dur = od.data_ptr() if od is not None else None
        a.lens = ld.data_ptr() if ld is not None else None
        a.ldl, a.bsl, a.B, a.T, a.nbins = nb, T * nb, Bn, T, nb
        L.check(lb.stzs_durations(a, None), "durations")
        torch.cuda.synchronize()
        return dur.cpu(), ds.cpu()

    dur, ds = run(logits, ov, LENS3)
    for b, n in enumerate(LENS3):
        d1, s1 = run(logits[b:b + 1, :n], None if ov is None else ov[b:b + 1, :n], None)
        assert torch.equal(dur[b, :n], d1[0]) and same_bits(ds[b, :n].contiguous(), s1[0].contiguous()), b
        assert bool((dur[b, n:] == 0).all()) and bool((ds[b, n:] == 0).all()), b
        assert bool((dur[b, :n] >= 1).all())


# ---- stzs_copy2d ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_copy2d_dst_row_off(lib, dtype):
    """block b of R rows lands at rows [off[b], off[b] + R) of its destination block (plain indexing), everything
    else keeps its bits; offsets NULL is the plain copy"""
    lb, L, dev = lib
    R, C, Td, ld = 4, 24, T6 + 4, 32
    dt, dti = (torch.bfloat16, L.BF16) if dtype == "bf16" else (torch.float32, L.F32)
    x = torch.randn(B3, R, C, generator=torch.Generator().manual_seed(2)).to(dt).to(dev)
    off = _i32(LENS3, dev)
    for offs in (LENS3, None):
        y = torch.full((B3, Td, ld), 5.0, dtype=dt, device=dev)
        a = L.CopyArgs()
        a.x, a.y, a.ldx, a.bsx, a.ldy, a.bsy = x.data_ptr(), y.data_ptr(), C, R * C, ld, Td * ld
        a.B, a.R, a.C, a.in_dtype, a.out_dtype = B3, R, C, dti, dti
        a.dst_row_off = off.data_ptr() if offs is not None else None
        L.check(lb.stzs_copy2d(a, None), "copy2d")
        torch.cuda.synchronize()
        want = torch.full((B3, Td, ld), 5.0, dtype=dt)
        for b in range(B3):
            o = offs[b] if offs is not None else 0
            want[b, o:o + R, :C] = x[b].cpu()
        assert same_bits(y.cpu(), want)
