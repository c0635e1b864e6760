"""Why row-local controls suffice, on the CPU in fp32 with the oracle, SPEC_TINY, seed-0 parameters and
the inputs of tests/test_gpu_ragged_frames_stages._inputs (B 4, T 12, seed 99).

  * guidance: the sampler restated over the batch on the CFG form with one scale per row
    (refops_controls.sample_style_rows) against oracle.sample_style on every row alone with cfg_scale = s_b, for
    s = [5, 1, 2.5, 0].  The figure is max-abs over max|ref| per row; the bound is that of
    tests/test_refops_ragged_frames.py (two formulations of the same fp32 arithmetic, batched against per row).  The
    s = 1 row is held against the cfg_scale = 1 run, which never builds the null-prompt rows;
  * rate: max(1, rint(dsum / r_b)) on the oracle's dsum for r = [1, 0.5, 1.7, 4.0]: the rows' frame counts are
    [48, 96, 24, 12] and no token's quotient lies within 0.12 of a rounding tie (dsum spans 3.81 - 4.04), so the
    guarded comparison of the GPU test has to excuse no token on these inputs.

Planted defects leave the bound: the rate applied after the rounding (other integers, other frame counts), the
conditional and unconditional predictions exchanged (orders of magnitude)."""
import pytest
import torch

import refops_controls as RC
from test_refops_ragged_frames import BOUND

SCALES = [5.0, 1.0, 2.5, 0.0]
RATES = [1.0, 0.5, 1.7, 4.0]
FRAMES = [48, 96, 24, 12]
STEPS = 2

_runs = {}


def _case(tiny, tiny_params):
    if not _runs:
        from oracle import stzs_ref as R
        from test_gpu_ragged_frames_stages import _inputs
        S, P = tiny, tiny_params
        h, codes = _inputs(S)
        g = torch.Generator().manual_seed(199)
        prompt = torch.randn(h.shape[0], S.L_s, S.code_dim, generator=g) * 0.3
        eps = torch.randn(h.shape[0], S.L_s, S.code_dim, generator=g)
        with torch.no_grad():
            solo = [R.sample_style(P, S, h[b:b + 1], prompt[b:b + 1], eps[b:b + 1], STEPS, s)[0]
                    for b, s in enumerate(SCALES)]
            pr = [R.predict_prosody(P, S, h[b:b + 1], codes[b:b + 1]) for b in range(h.shape[0])]
        dsum = torch.cat([p["dur_sum"] for p in pr])
        _runs.update(R=R, h=h, codes=codes, prompt=prompt, eps=eps, solo=solo, dsum=dsum,
                     dur_pred=torch.cat([p["dur_pred"] for p in pr]))
    return _runs


def _worst(c, got):
    worst = []
    for b, want in enumerate(c["solo"]):
        worst.append(((got[b] - want).abs().max() / want.abs().max()).item())
    return worst


def test_per_row_scale_matches_rows_alone(tiny, tiny_params):
    c = _case(tiny, tiny_params)
    with torch.no_grad():
        got = RC.sample_style_rows(c["R"], tiny_params, tiny, c["h"], c["prompt"], c["eps"], STEPS, SCALES)
    w = _worst(c, got)
    print("per-row scale, max-abs / max|ref| per row:", ["%.2e" % v for v in w], f"(bound {BOUND:.2e})")
    assert max(w) <= BOUND
    assert SCALES[1] == 1.0  # (that row's reference above is the cfg_scale = 1 run: no null-prompt rows at all)


def test_exchanged_predictions_leave_the_bound(tiny, tiny_params):
    c = _case(tiny, tiny_params)
    with torch.no_grad():
        got = RC.sample_style_rows(c["R"], tiny_params, tiny, c["h"], c["prompt"], c["eps"], STEPS, SCALES, "swapped")
    w = _worst(c, got)
    print("exchanged predictions:", ["%.2e" % v for v in w])
    assert max(w) > 100 * BOUND


def test_duration_rule_and_frame_counts(tiny, tiny_params):
    c = _case(tiny, tiny_params)
    dsum = c["dsum"]
    print(f"dsum spans {float(dsum.min()):.2f} - {float(dsum.max()):.2f}")
    want = torch.clamp(torch.round(dsum / torch.tensor(RATES)[:, None]), min=1).to(torch.int32)
    got = RC.durations_with_rate(dsum, RATES)
    assert torch.equal(got, want)
    assert got.sum(1).tolist() == FRAMES
    assert torch.equal(got[0], c["dur_pred"][0])  # rate 1: the rule without a rate
    dist = RC.tie_distance(dsum, RATES)
    print(f"nearest quotient to a rounding tie: {dist:.3f}")
    assert dist > 0.12
    assert int(RC.quotient_ties(dsum, RATES, 1e-3).sum()) == 0  # the GPU test's guard excuses no token here


def test_rate_after_rounding_leaves_the_bound(tiny, tiny_params):
    """the planted defect: the rate applied to the rounded sum.  On RATES it cannot show -- every dsum rounds to 4 and
    rint(4 / r) is rint(dsum / r) for r in {1, 0.5, 1.7, 4.0} -- so it is planted on rates that separate the two on the
    same dsum: 0.25 (3.81 / 0.25 = 15.2 against 16) and 0.7 (5.44 against 5.71)."""
    c = _case(tiny, tiny_params)
    assert torch.equal(RC.durations_with_rate(c["dsum"], RATES, "after_rounding"), RC.durations_with_rate(c["dsum"], RATES))
    rates = [0.25, 0.7, 0.25, 0.7]
    good, bad = RC.durations_with_rate(c["dsum"], rates), RC.durations_with_rate(c["dsum"], rates, "after_rounding")
    print("rate after rounding: frame counts", bad.sum(1).tolist(), "against", good.sum(1).tolist())
    assert int((good != bad).sum()) > 0
    assert good.sum(1).tolist() != bad.sum(1).tolist()


def test_pitch_factor_is_the_float64_power():
    for p, want in ((0.0, 1.0), (12.0, 2.0), (-12.0, 0.5), (24.0, 4.0), (-24.0, 0.25)):
        assert float(RC.pitch_factor(p)) == want
    assert float(RC.pitch_factor(7.0)) == float(torch.tensor(2.0 ** (7.0 / 12.0), dtype=torch.float64).float())
    assert RC.pitch_factor(1.0).dtype == torch.float32
