"""The LSTM recurrence (csrc/lstm.hip) element by element, straight through the C ABI (stzs_lstm / stzs_lstm_pair)
against the teacher-forced fp64 reference of tests/refops.py (lstm_tf_ref: the kernel's own stored y as h_{t-1}, only
the cell state carried, a running per-element error bound; validated on the CPU by tests/test_refops_lstm.py).

Every case must give ratio = max |y - h_ref| / bound <= 1 and, for bf16 output, at most 1 % of the elements off the
reference's own bf16 rounding (lstm_tf_check); both numbers are printed.  After EVERY launch the status word is 0 and
the 1024 sync words and the granule region (the first TAG_BYTES of xchg) read back as zeros -- the kernel's
leave-it-zeroed contract -- and every output buffer is allocated with guard rows and columns of a NaN bit pattern that
must survive.  The cases name the kernel instantiation lstm_xchg<NKS = H / 32, PR = precise, GR> they launch; the
group height GR is asserted from the rule of lstm_group_rows restated here, from stzs_lstm_workspace, and from where
the last two steps' h lie in the exchange slab ([group][dir][parity][GR][NH H] behind the granules)."""
import math

import pytest
import torch

from refops import _bits, fill_bits, lstm_tf_check, lstm_tf_ref, same_bits

pytestmark = pytest.mark.gpu

TAG_ROWS, TAG_BYTES = 2, 8192            # csrc/lstm.hip: groups of <= 2 rows exchange tagged granules (bf16 mode)
NAN = {torch.bfloat16: 0x7FC5, torch.float32: 0x7FC00005}  # guard fill: a quiet NaN with a payload


def group_rows(B, H, ndir):
    """csrc/lstm.hip lstm_group_rows: one 64-row group up to 16 utterances, else the smallest of 16 / 32 / 64 rows
    that keeps groups x directions <= 63 and the grid <= 256 workgroups"""
    if B <= 16:
        return 64
    gr = 16
    while gr < 64:
        g = -(-B // gr)
        if g * ndir <= 63 and (H // 32) * ndir * g <= 256:
            return gr
        gr *= 2
    return 64


@pytest.fixture(scope="module")
def lib(gpu_device):
    from stzs import _lib as L
    return L.load(), L, gpu_device


_W = {}


def _weights(H, precise, dev):
    """W_hh of both directions, uniform in +-1 / sqrt(H) -> (as the kernel holds them, for lstm_tf_ref; the device
    fragments in the documented two-direction layout: [dir] bf16 fragments, precise: [hi | lo][dir])"""
    from stzs.weights import lstm_frags, split_bf16
    if (H, precise) not in _W:
        g = torch.Generator().manual_seed(7 + H)
        w = [(torch.rand(4 * H, H, generator=g) * 2 - 1) / math.sqrt(H) for _ in range(2)]
        if precise:
            held = [split_bf16(v) for v in w]
            fr = torch.stack([torch.stack([lstm_frags(held[d][h].float()) for d in range(2)], 0) for h in range(2)], 0)
        else:
            held = [v.to(torch.bfloat16).float() for v in w]
            fr = torch.stack([lstm_frags(v) for v in held], 0)
        _W[(H, precise)] = (held, fr.to(torch.bfloat16).contiguous().to(dev))
    return _W[(H, precise)]


def _gx(B, T, H, seed):
    return 1.5 * torch.randn(B, T, 8 * H, generator=torch.Generator().manual_seed(seed))


class _Run:
    """one recurrence's launch state.  gx [B, T, 8H] sits in a buffer of row pitch 8H + gpad, y in a buffer [B, T +
    yrows, 2H + ycols]; both start as the NaN fill, so what the kernel does not write -- or reads where it must not --
    shows.  Its own exchange workspace, sync words and status word, zeroed once."""

    def __init__(self, lb, L, dev, whh, gx, H, precise, lens=None, ndir=2, yrows=1, ycols=8, gpad=0):
        self.B, self.T, self.H, self.ndir, self.precise = gx.shape[0], gx.shape[1], H, ndir, precise
        B, T = self.B, self.T
        self.ydt = torch.float32 if precise else torch.bfloat16
        gbuf = fill_bits((B, T, 8 * H + gpad), torch.float32, NAN[torch.float32])
        gbuf[:, :, :8 * H] = gx
        self.gx = gbuf.to(dev)
        self.ybuf = fill_bits((B, T + yrows, 2 * H + ycols), self.ydt, NAN[self.ydt], dev)
        self.ws = lb.stzs_lstm_workspace(B, H, ndir)
        self.xchg = torch.zeros(self.ws, dtype=torch.uint8, device=dev)
        self.sync = torch.zeros(1024, dtype=torch.int32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        a = self.a = L.LstmArgs()
        a.gx, a.whhT, a.y, a.xchg, a.sync = (t.data_ptr() for t in (self.gx, whh, self.ybuf, self.xchg, self.sync))
        a.ldg, a.bsg = 8 * H + gpad, T * (8 * H + gpad)
        a.ldy, a.bsy = 2 * H + ycols, (T + yrows) * (2 * H + ycols)
        a.B, a.T, a.H, a.ndir, a.precise = B, T, H, ndir, precise
        a.status = self.status.data_ptr()
        a.lens = self.lens.data_ptr() if self.lens is not None else None

    def done(self):
        """-> y [B, T, ndir H] on the CPU, after the contract checks of every launch"""
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0, "LSTM exchange timed out"
        assert not bool(self.sync.any()), f"sync words left set: {self.sync.nonzero().flatten().tolist()[:8]}"
        assert not bool(self.xchg[:TAG_BYTES].any()), "granule region not left zeroed"
        buf = self.ybuf.cpu()
        T, W = self.T, self.ndir * self.H
        probe, fill = buf.clone(), fill_bits(buf.shape, self.ydt, NAN[self.ydt])
        probe[:, :T, :W] = fill[:, :T, :W]
        assert same_bits(probe, fill), "y written outside [B, T, ndir H]"
        y = buf[:, :T, :W].contiguous()
        assert bool(torch.isfinite(y.float()).all()), "y holds unwritten or non-finite elements"
        return y

    def assert_group_rows(self, gr, y):
        """the launch ran at group height gr: the rule, the workspace size, and the slab rows of the last two steps
        (bf16 mode: the bits of y; precise: hi = bf16(y) | lo = bf16(y - hi)) lie where that height puts them"""
        B, T, H, ndir = self.B, self.T, self.H, self.ndir
        assert group_rows(B, H, ndir) == gr
        groups = -(-B // gr)
        assert self.ws == TAG_BYTES + groups * ndir * 2 * gr * 2 * H * 2
        nh = 2 if self.precise else 1
        slab = self.xchg[TAG_BYTES:].cpu().view(torch.bfloat16)[:groups * ndir * 2 * gr * nh * H]
        slab = slab.view(groups, ndir, 2, gr, nh * H)
        for s in (T - 1, T - 2):
            for d in range(ndir):
                yt = y[:, s if d == 0 else T - 1 - s, d * H:(d + 1) * H]
                hi = yt.to(torch.bfloat16)
                want = torch.cat([hi, (yt.float() - hi.float()).to(torch.bfloat16)], 1) if self.precise else hi
                for g in range(groups):
                    n = min(gr, B - g * gr)
                    if not self.precise and n <= TAG_ROWS:
                        continue  # a tagged group hands h over as granules, not through the slab
                    assert torch.equal(_bits(slab[g, d, s & 1, :n]), _bits(want[g * gr:g * gr + n])), (s, d, g)


def _launch(lib, whh, gx, H, precise, **kw):
    lb, L, dev = lib
    r = _Run(lb, L, dev, whh, gx, H, precise, **kw)
    L.check(lb.stzs_lstm(r.a, None), "lstm")
    return r, r.done()


def _parity(name, gx, held, y, H, ndir, precise, lens=None):
    ratio, share = lstm_tf_check(y, *lstm_tf_ref(gx, held, y, H, ndir, lens, bool(precise)), not precise)
    print(f"lstm parity {name} ({'precise' if precise else 'bf16'}): ratio {ratio:.4f}, flip share {share:.2e}")
    assert ratio <= 1, f"{name}: |y - h_ref| reaches {ratio:.3f} x its bound"
    assert share <= 0.01, f"{name}: {share:.3%} of the elements are off the reference's bf16 rounding"


# group class -> (B at H <= 128, B at H = 256, T, group height)
CLASSES = {"one-tile": (3, 3, 7, 64), "gr16": (40, 40, 7, 16), "gr32": (500, 270, 4, 32), "gr64": (1000, 520, 4, 64)}


@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("H", [32, 64, 128, 256])
def test_every_instantiation(lib, H, precise, cls):
    """lstm_xchg<H / 32, precise, GR> for all 24 (NKS, PR, GR).  GR = 64 runs as one tile (B = 3) and as tall groups (B =
    1000: 15 groups of 4 row tiles, both wave halves, and a last group of 40 rows whose upper wave half runs one tile of
    its two; H = 256: B = 520, last group 8 rows); GR = 16 at B = 40 (16, 16, 8 rows); GR = 32 at B = 500 (the last group
    has 20 rows: a partly filled second tile; H = 256: B = 270, last group 14 rows).  T = 7 reuses both slab parities."""
    Bs, B8, T, gr = CLASSES[cls]
    B = B8 if H == 256 else Bs
    held, whh = _weights(H, precise, lib[2])
    gx = _gx(B, T, H, 1000 * H + B)
    r, y = _launch(lib, whh, gx, H, precise)
    r.assert_group_rows(gr, y)
    _parity(f"H{H} {cls} B{B} T{T}", gx, held, y, H, 2, precise)


@pytest.mark.parametrize("B", [1, 2, 17, 18])
@pytest.mark.parametrize("H", [128, 256])
def test_tagged_and_mixed(lib, H, B):
    """bf16 mode, T = 9: B = 1 / 2 exchange tagged granules; at B = 17 / 18 the first group of 16 uses the counters
    and the last group of 1 / 2 rows is tagged, in one launch"""
    held, whh = _weights(H, 0, lib[2])
    gx = _gx(B, 9, H, 77 * H + B)
    r, y = _launch(lib, whh, gx, H, 0)
    assert min(16, B - (B - 1) // 16 * 16) <= TAG_ROWS  # (the last group's rows: this case does run the tagged form)
    r.assert_group_rows(64 if B <= 16 else 16, y)
    _parity(f"H{H} tagged B{B} T9", gx, held, y, H, 2, 0)


@pytest.mark.parametrize("precise", [0, 1])
def test_ragged_rows_beyond_first_tile(lib, precise):
    """GR = 32, H = 32, B = 500, random lens in [1, T] with lengths 1 and T forced into rows >= 16 of the first and the
    last group (the cells of the second row tile look up their own clen): parity with lens, exact zeros past them"""
    H, B, T = 32, 500, 7
    lens = torch.randint(1, T + 1, (B,), generator=torch.Generator().manual_seed(5)).tolist()
    for b, n in ((0, T), (16, 1), (17, T), (31, 1), (480 + 16, 1), (480 + 17, T), (480 + 19, 1)):
        lens[b] = n
    held, whh = _weights(H, precise, lib[2])
    gx = _gx(B, T, H, 31)
    r, y = _launch(lib, whh, gx, H, precise, lens=lens)
    r.assert_group_rows(32, y)
    for b, n in enumerate(lens):
        assert bool((y[b, n:] == 0).all()), f"row {b}: y past its length {n} is not zero"
        assert bool((y[b, :n] != 0).any(-1).all()), f"row {b}: a kept step is all zeros"
    _parity("H32 gr32 ragged B500 T7", gx, held, y, H, 2, precise, lens)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("precise", [0, 1])
def test_one_direction(lib, precise, B):
    """ndir = 1 with the two-direction whhT and an ldg = 8H gx (include/stzs.h): y[:, :, :H] is the bits of the forward
    half of the ndir = 2 launch, columns [H, 2H) of the NaN-filled y are untouched (checked in done()), and the output
    satisfies the reference.  B = 2 is the tagged form in bf16 mode, B = 3 the counter form."""
    H, T = 64, 7
    held, whh = _weights(H, precise, lib[2])
    gx = _gx(B, T, H, 900 + B)
    _, y2 = _launch(lib, whh, gx, H, precise)
    r, y1 = _launch(lib, whh, gx, H, precise, ndir=1)
    assert y1.shape == (B, T, H) and same_bits(y1, y2[:, :, :H].contiguous())
    r.assert_group_rows(64, y1)
    _parity(f"H64 ndir1 B{B} T7", gx[:, :, :4 * H], held[:1], y1, H, 1, precise)


@pytest.mark.parametrize("B", [3, 2])
@pytest.mark.parametrize("precise", [0, 1])
def test_guards(lib, precise, B):
    """y with ldy = 2H + 8 and bsy = (T + 2) ldy, gx with ldg = 8H + 8, all padding a NaN bit pattern: the logical region
    passes the check (no NaN was read into it) and the rest of the y buffer keeps its fill bit for bit (done())"""
    H, T = 64, 7
    held, whh = _weights(H, precise, lib[2])
    gx = _gx(B, T, H, 500 + B)
    r, y = _launch(lib, whh, gx, H, precise, yrows=2, ycols=8, gpad=8)
    assert (r.a.ldy, r.a.bsy, r.a.ldg) == (2 * H + 8, (T + 2) * (2 * H + 8), 8 * H + 8)
    _parity(f"H64 guards B{B} T7", gx, held, y, H, 2, precise)


@pytest.mark.parametrize("precise", [0, 1])
def test_pair_tall_group(lib, precise):
    """stzs_lstm_pair at H = 32, B = 500 with T = 4 and T = 6: GR = 32, 2 x 32 workgroups in one launch; each output is
    the bits of its own stzs_lstm call and the first satisfies the reference"""
    lb, L, dev = lib
    H, B = 32, 500
    held, whh = _weights(H, precise, dev)
    gxa, gxb = _gx(B, 4, H, 61), _gx(B, 6, H, 62)
    (_, ya), (_, yb) = _launch(lib, whh, gxa, H, precise), _launch(lib, whh, gxb, H, precise)
    pa, pb = _Run(lb, L, dev, whh, gxa, H, precise), _Run(lb, L, dev, whh, gxb, H, precise)
    L.check(lb.stzs_lstm_pair(pa.a, pb.a, None), "lstm_pair")
    za, zb = pa.done(), pb.done()
    assert same_bits(za, ya) and same_bits(zb, yb)
    pa.assert_group_rows(32, za)
    pb.assert_group_rows(32, zb)
    _parity("H32 pair B500 T4", gxa, held, za, H, 2, precise)
