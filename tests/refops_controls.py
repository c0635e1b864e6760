"""CPU restatements of the per-request controls for the tests: the batched sampler with one guidance
scale per row, the duration rule with a speaking rate, the pitch factor, and the tie guard on the quotients.  Everything
here is fp32 torch on the host, built on the oracle's own functions (passed in as R)."""
import torch


def sample_style_rows(R, P, S, h_txt, prompt, eps, steps, scales, defect=None):
    """oracle.stzs_ref.sample_style on the CFG form (2B rows, null-prompt context) with row b's own scale:
    d = (s_b == 1) ? D_c : D_u + s_b (D_c - D_u), then the Euler update.  scales: B floats.
    defect "swapped": the conditional and the unconditional prediction exchanged."""
    B = h_txt.shape[0]
    s = torch.tensor([float(v) for v in scales], dtype=torch.float32)[:, None, None]
    kv, pool = R.denoiser_context(P, S, h_txt, prompt, True)
    sig = R.sigma_schedule(S, steps)
    x = eps * sig[0]
    for i in range(steps):
        D = R.denoiser(P, S, torch.cat([x, x], 0), sig[i], kv, pool)
        dc, du = (D[B:], D[:B]) if defect == "swapped" else (D[:B], D[B:])
        d = torch.where(s == 1, dc, du + s * (dc - du))
        x = x + (sig[i + 1] - sig[i]) * (x - d) / sig[i]
    return x


def durations_with_rate(dsum, rate, defect=None):
    """dsum fp32 [B, T] (the raw sigmoid sums), rate B floats -> int32 [B, T]: max(1, rint(dsum / r_b)), the quotient
    one fp32 division (torch's is correctly rounded).  defect "after_rounding": the rate applied to the rounded sum."""
    r = torch.tensor([float(v) for v in rate], dtype=torch.float32)[:, None]
    dsum = dsum.to(torch.float32)
    q = torch.round(dsum) / r if defect == "after_rounding" else dsum / r
    return torch.clamp(torch.round(q), min=1).to(torch.int32)


def device_rate(rate):
    """what the durations kernel makes of a rate: not finite or <= 0 -> 1"""
    return [float(v) if (v == v and 0.0 < v < float("inf")) else 1.0 for v in rate]


def pitch_factor(p):
    """float32(2.0 ** (p / 12)), the power in float64"""
    return torch.tensor(2.0 ** (float(p) / 12.0), dtype=torch.float64).to(torch.float32)


def quotient_ties(dsum_ref, rate, err):
    """the tokens whose reference quotient dsum / r_b lies within err + 1e-4 of a rounding tie k + 0.5 (the guard of
    tests/test_gpu_configs.py _dur_guarded_equal, applied to the quotients) -> bool [B, T]"""
    q = dsum_ref.to(torch.float32) / torch.tensor([float(v) for v in rate], dtype=torch.float32)[:, None]
    return (q - q.floor() - 0.5).abs() <= err + 1e-4


def tie_distance(dsum_ref, rate):
    """the smallest distance of any token's quotient from a rounding tie"""
    q = dsum_ref.to(torch.float32) / torch.tensor([float(v) for v in rate], dtype=torch.float32)[:, None]
    return float((q - q.floor() - 0.5).abs().min())
