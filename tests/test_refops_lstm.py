"""CPU self-checks of the LSTM references in tests/refops.py (used by tests/test_gpu_lstm_parity.py): the teacher-forced
fp64 reference against torch.nn.LSTM in double and a hand-written recurrence, its ragged rule, the precise mode's
operand split, the per-element bound on an honest fp32 emulation of the kernel (lstm_emulate), and the same check
going red on emulations with one mistake each."""
import math

import pytest
import torch

from refops import half_ulp_bf16, lstm_emulate, lstm_tf_check, lstm_tf_ref, round_bf16, split_hi_lo

# (H, B, T): one to eight K-steps, one and several row tiles, a long recurrence
SHAPES = [(32, 40, 7), (128, 3, 7), (256, 20, 9), (64, 3, 60)]
MUTATIONS = ["w", "swap_if", "stale", "zero_row", "c_drift"]


def _case(H, B, T, ndir=2, precise=False, seed=0):
    """the GPU file's operands: gx = 1.5 randn, W_hh uniform in +-1 / sqrt(H) as the kernel holds it, random lens"""
    from stzs.weights import split_bf16
    g = torch.Generator().manual_seed(seed + 1000 * H + 10 * B + T)
    gx = 1.5 * torch.randn(B, T, ndir * 4 * H, generator=g)
    w = [(torch.rand(4 * H, H, generator=g) * 2 - 1) / math.sqrt(H) for _ in range(ndir)]
    w = [split_bf16(v) for v in w] if precise else [v.to(torch.bfloat16).float() for v in w]
    lens = torch.randint(1, T + 1, (B,), generator=g).tolist()
    return gx, w, lens


_CASES = {}


def _shared(shape):
    """operands of a shape and the clean emulation's verdict, computed once"""
    if shape not in _CASES:
        H, B, T = shape
        gx, w, lens = _case(H, B, T)
        y = lstm_emulate(gx, w, H, 2, lens)
        _CASES[shape] = (gx, w, lens, lstm_tf_check(y, *lstm_tf_ref(gx, w, y, H, 2, lens), True))
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d-B%d-T%d" % s)
def test_clean_model_passes(shape):
    ratio, share = _shared(shape)[3]
    print(f"lstm emulation {shape}: ratio {ratio:.3f}, flip share {share:.2e}")
    assert ratio <= 1 and share <= 0.01


@pytest.mark.parametrize("mutate", MUTATIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d-B%d-T%d" % s)
def test_mutation_fails(shape, mutate):
    """every one-mistake emulation fails the ratio or the flip share, at every shape"""
    H, B, T = shape
    gx, w, lens, _ = _shared(shape)
    y = lstm_emulate(gx, w, H, 2, lens, mutate)
    ratio, share = lstm_tf_check(y, *lstm_tf_ref(gx, w, y, H, 2, lens), True)
    print(f"lstm emulation {shape} with '{mutate}': ratio {ratio:.3g}, flip share {share:.2e}")
    assert ratio > 1 or share > 0.01


@pytest.mark.parametrize("shape", [(32, 5, 7), (64, 3, 9)], ids=lambda s: "H%d-B%d-T%d" % s)
def test_precise_model(shape):
    """the split-operand emulation (fp32 y) passes with bound = E_h alone; one W_hh element off by 0.05 does not"""
    H, B, T = shape
    gx, w, lens = _case(H, B, T, precise=True)
    y = lstm_emulate(gx, w, H, 2, lens, precise=True)
    ratio, _ = lstm_tf_check(y, *lstm_tf_ref(gx, w, y, H, 2, lens, precise=True), False)
    ym = lstm_emulate(gx, w, H, 2, lens, "w", precise=True)
    bad, _ = lstm_tf_check(ym, *lstm_tf_ref(gx, w, ym, H, 2, lens, precise=True), False)
    print(f"precise lstm emulation {shape}: ratio {ratio:.3f}; with 'w': {bad:.3g}")
    assert ratio <= 1 < bad


def test_teacher_forcing_reproduces_free_running_fp64():
    """A free-running nn.LSTM in double, stepped one position at a time with its h rounded to bf16 before every step
    (c untouched): fed that rounded output, lstm_tf_ref gives the UNROUNDED h of every step to fp64 rounding -- and so
    does a hand-written fp64 recurrence of the textbook equations (forward only)."""
    H, B, T, In = 32, 3, 11, 16
    torch.manual_seed(3)
    net = torch.nn.LSTM(In, H, batch_first=True).double()
    x = torch.randn(B, T, In, dtype=torch.float64)
    w_ih, w_hh = net.weight_ih_l0.detach(), net.weight_hh_l0.detach()
    gx = x @ w_ih.t() + net.bias_ih_l0.detach() + net.bias_hh_l0.detach()
    rb = lambda v: round_bf16(v).double()
    h, c = torch.zeros(1, B, H, dtype=torch.float64), torch.zeros(1, B, H, dtype=torch.float64)
    hh, ch = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
    raw, hand = [], []
    with torch.no_grad():
        for t in range(T):
            o, (h, c) = net(x[:, t:t + 1], (rb(h), c))
            raw.append(o[:, 0])
            i, f, g, oo = (gx[:, t] + rb(hh) @ w_hh.t()).split(H, 1)
            ch = torch.sigmoid(f) * ch + torch.sigmoid(i) * torch.tanh(g)
            hh = torch.sigmoid(oo) * torch.tanh(ch)
            hand.append(hh)
    raw, hand = torch.stack(raw, 1), torch.stack(hand, 1)
    h_ref, E_h = lstm_tf_ref(gx, [w_hh], round_bf16(raw), H, 1)
    assert (h_ref - raw).abs().max().item() < 1e-13 and (h_ref - hand).abs().max().item() < 1e-13
    assert bool((E_h > 0).all()) and E_h.max().item() < 1e-4


def test_ragged_rows():
    """lens [1, T, 4]: row b of the reference at t < lens[b] is that row alone at T = lens[b] (the reverse direction
    starts at the row's own last position from the zero state), and h_ref = E_h = 0 past it; lengths are clamped into
    [1, T]"""
    H, T, lens = 32, 7, [1, 7, 4]
    gx, w, _ = _case(H, 3, T)
    y = lstm_emulate(gx, w, H, 2, lens)
    h_ref, E_h = lstm_tf_ref(gx, w, y, H, 2, lens)
    for b, n in enumerate(lens):
        assert bool((y[b, n:] == 0).all() and (h_ref[b, n:] == 0).all() and (E_h[b, n:] == 0).all())
        solo = lstm_emulate(gx[b:b + 1, :n], w, H, 2)
        assert torch.equal(solo[0], y[b, :n])
        hs, Es = lstm_tf_ref(gx[b:b + 1, :n], w, solo, H, 2)
        assert torch.equal(hs[0], h_ref[b, :n]) and torch.equal(Es[0], E_h[b, :n])
    # the reverse direction's first step of the one-token row starts from zeros: its h depends on gx[1, 0] alone
    i, f, g, o = gx[0, 0, 4 * H:].double().split(H)
    assert torch.allclose(h_ref[0, 0, H:], torch.sigmoid(o) * torch.tanh(torch.sigmoid(i) * torch.tanh(g)), atol=1e-15)
    for bad in ([0, 9, 4], [-3, 7, 4]):
        hc, Ec = lstm_tf_ref(gx, w, y, H, 2, bad)
        assert torch.equal(hc, h_ref) and torch.equal(Ec, E_h)
    # a tail that is not exactly zero is an infinite ratio
    y2 = y.clone()
    y2[0, 3, 5] = 1e-30
    assert lstm_tf_check(y2, h_ref, E_h, True)[0] == float("inf")


def test_precise_split():
    """hi + lo reconstructs y to 2^-16 |y|, hi is the bf16 rounding and both parts are bf16 values"""
    y = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * torch.logspace(-6, 2, 4096)
    hi, lo = split_hi_lo(y)
    assert bool(((hi + lo - y.double()).abs() <= 2.0 ** -16 * y.double().abs()).all())
    assert torch.equal(hi, y.to(torch.bfloat16).double())
    assert torch.equal(lo, lo.to(torch.bfloat16).double())


def test_half_ulp_bf16():
    h = torch.tensor([1.0, 1.5, 1.999, 2.0, -0.3, 0.0, 1.0 - 2.0 ** -10], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -10, 0.0, 2.0 ** -8], dtype=torch.float64)
    assert torch.equal(half_ulp_bf16(h), want)
