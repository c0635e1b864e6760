"""Mixed-length traffic through BucketScheduler with and without ragged_text (DESIGN.md "Ragged text batches").

64 requests on SPEC_V0: token counts drawn with a fixed seed from 20..200, 3-s references, 2 steps, CFG 5, predicted
durations.  One engine, the same requests; ragged_text=False (the schedule without the feature: the baseline) and
True are timed in alternation after a warm-up of each -- a host clock around synth() ending in a device
synchronise -- and the medians, the phase-1 batch counts and the phase-1 wall time (each phase-1 batch ends in a
host sync, so the scheduler's own clock is the phase's) go out as one JSON line.

    python tools/ragged_traffic.py [--requests 64] [--runs 7] [--warmup 2] [--mode both|plain|ragged]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "styletts-zs_amd")]
import torch  # noqa: E402

STEPS, CFG, REF_S, TOK_LO, TOK_HI, SEED = 2, 5.0, 3.0, 20, 200, 2024


def make_requests(S, n, seed=SEED):
    from stzs.scheduler import Request
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(TOK_LO, TOK_HI + 1, (n,), generator=g).tolist()
    return [Request(tokens=torch.randint(1, S.n_symbols, (T,), generator=g),
                    ref_wav=torch.randn(int(REF_S * S.sr), generator=g) * 0.1,
                    noise=torch.randn(S.L_s, S.code_dim, generator=g), seed=k) for k, T in enumerate(lens)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--mode", choices=("both", "plain", "ragged"), default="both")
    a = ap.parse_args()
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.scheduler import BucketScheduler
    from stzs.spec import SPEC_V0 as S
    if not torch.cuda.is_available():
        raise SystemExit("ragged_traffic.py measures on the GPU: none is visible")
    eng = StyleTTSZS(S, init_params(S, seed=0), device="cuda:0")
    reqs = make_requests(S, a.requests)
    modes = {"plain": False, "ragged": True}
    if a.mode != "both":
        modes = {a.mode: modes[a.mode]}
    sch = {m: BucketScheduler(eng, max_batch=a.max_batch, steps=STEPS, cfg_scale=CFG, ragged_text=r)
           for m, r in modes.items()}
    wall = {m: [] for m in sch}
    ph1 = {m: [] for m in sch}
    outs = {}

    def run(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = sch[m].synth(reqs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, o

    for m in sch:
        for _ in range(a.warmup):
            _, outs[m] = run(m)
    for _ in range(a.runs):  # alternating: what shares the host moves both alike
        for m in sch:
            dt, _ = run(m)
            wall[m].append(1e3 * dt)
            ph1[m].append(sch[m].stats["phase1_ms"])
    res = dict(requests=a.requests, tokens=[int(r.tokens.shape[0]) for r in reqs], steps=STEPS, cfg=CFG, ref_s=REF_S,
               runs=a.runs, warmup=a.warmup)
    for m in sch:
        st = sch[m].stats
        res[m] = dict(phase1_batches=st["phase1_batches"], phase2_batches=st["phase2_batches"],
                      wall_ms_median=round(statistics.median(wall[m]), 2), wall_ms_min=round(min(wall[m]), 2),
                      wall_ms_max=round(max(wall[m]), 2), phase1_ms_median=round(statistics.median(ph1[m]), 2),
                      phase1_ms_min=round(min(ph1[m]), 2), phase1_ms_max=round(max(ph1[m]), 2))
    if len(sch) == 2:  # the two schedules computed the same waveforms
        worst = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(outs["ragged"], outs["plain"]))
        res["max_rel_diff_ragged_vs_plain"] = worst
    print(json.dumps(res))


if __name__ == "__main__":
    main()
