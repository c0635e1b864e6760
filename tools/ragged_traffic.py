"""Mixed-length traffic through BucketScheduler with and without ragged_text / ragged_ref (DESIGN.md "Ragged text
batches" and §2c "Ragged reference batches").

64 requests on SPEC_V0: token counts drawn with a fixed seed from 20..200, 3-s references (--ref-s LO,HI: reference
lengths drawn with the same seed, uniformly in samples, from LO..HI seconds), 2 steps, CFG 5, predicted durations.
One engine, the same requests; the schedules -- plain (neither flag: the baseline), ragged (ragged_text=True),
ragged_ref (ragged_text=True and ragged_ref=True), ragged_frames (those and ragged_frames: prosody in one ragged batch
per max_batch requests) and ragged_decoder (all four flags: the decoder too runs one ragged pass per
max_batch requests, sorted by frame count) -- are timed in alternation after a warm-up of each -- a host clock
around synth() ending in a device synchronise -- and the medians, the phase-1 batch counts, the phase-1 wall time
(each phase-1 batch ends in a host sync, so the scheduler's own clock is the phase's) and the share of the phase-1
reference blocks that is padding go out as one JSON line.

    python tools/ragged_traffic.py [--requests 64] [--runs 7] [--warmup 2] [--ref-s LO,HI] [--engine default|precise]
                                   [--mode both|all|plain|ragged|ragged_ref|ragged_frames|ragged_decoder|controls]

--engine precise: the same protocol on StyleTTSZS(precise=True), whose convs take the lengths on the
mrfx / conv_x3 forms.

--mode both: plain and ragged (the measurement of "Ragged text batches"); all: the five schedules.

--mode controls: the same 64 requests each draw, seeded, one of four guidance scales (CONTROL_SCALES) and
a speaking rate uniform in 0.8 .. 1.25.  Two ways to serve them, both with all four ragged flags, timed in alternation:
`controls`, ONE scheduler with the per-request controls, and `per_scale`, what there was before them -- one scheduler
per distinct guidance scale on the requests that share it, the rates not expressible (every request at rate 1, so it
computes other waveforms: the comparison is of batches and wall time).  Batch counts and the medians go out as one
JSON line.
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
CONTROL_SCALES, RATE_LO, RATE_HI = (1.0, 2.5, 5.0, 7.5), 0.8, 1.25


def make_requests(S, n, seed=SEED, ref_s=None):
    """ref_s = (lo, hi) seconds: per-request reference lengths, seeded, uniform in samples; None: REF_S for all (the
    request stream is then the one this tool always made)"""
    from stzs.scheduler import Request
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(TOK_LO, TOK_HI + 1, (n,), generator=g).tolist()
    nref = [int(REF_S * S.sr)] * n
    if ref_s is not None:
        lo, hi = int(ref_s[0] * S.sr), int(ref_s[1] * S.sr)
        nref = torch.randint(lo, hi + 1, (n,), generator=torch.Generator().manual_seed(seed + 1)).tolist()
    return [Request(tokens=torch.randint(1, S.n_symbols, (T,), generator=g),
                    ref_wav=torch.randn(nref[k], generator=g) * 0.1,
                    noise=torch.randn(S.L_s, S.code_dim, generator=g), seed=k) for k, T in enumerate(lens)]


def draw_controls(n, seed=SEED + 2):
    """-> ([guidance scale], [rate]) of n requests, seeded: a scale of CONTROL_SCALES, a rate in RATE_LO .. RATE_HI"""
    g = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, len(CONTROL_SCALES), (n,), generator=g).tolist()
    rate = (RATE_LO + (RATE_HI - RATE_LO) * torch.rand(n, generator=g, dtype=torch.float64)).tolist()
    return [CONTROL_SCALES[k] for k in pick], [round(r, 3) for r in rate]


def controls_mode(a, eng, S, reqs):
    """one scheduler with per-request controls against one scheduler per guidance scale -> the result dict"""
    import copy
    from stzs.scheduler import BucketScheduler
    scales, rates = draw_controls(len(reqs))
    flags = dict(ragged_text=True, ragged_ref=True, ragged_frames=True, ragged_decoder=True)
    mixed = [copy.copy(r) for r in reqs]
    for r, s, v in zip(mixed, scales, rates):
        r.cfg_scale, r.speed = s, v
    one = BucketScheduler(eng, max_batch=a.max_batch, steps=STEPS, cfg_scale=CFG, **flags)
    per = {s: (BucketScheduler(eng, max_batch=a.max_batch, steps=STEPS, cfg_scale=s, **flags),
               [r for r, q in zip(reqs, scales) if q == s]) for s in sorted(set(scales))}

    def run_controls():
        one.synth(mixed)
        st = one.stats
        return st["phase1_batches"], st["phase2_batches"], st["control_batches"]

    def run_per_scale():
        n1 = n2 = 0
        for sch, sub in per.values():
            sch.synth(sub)
            n1, n2 = n1 + sch.stats["phase1_batches"], n2 + sch.stats["phase2_batches"]
        return n1, n2, 0

    ways = {"controls": run_controls, "per_scale": run_per_scale}
    wall, counts = {m: [] for m in ways}, {}

    def timed(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts[m] = ways[m]()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for m in ways:
        for _ in range(a.warmup):
            timed(m)
    for _ in range(a.runs):
        for m in ways:
            wall[m].append(timed(m))
    res = dict(mode="controls", requests=len(reqs), steps=STEPS, scales=list(CONTROL_SCALES), rate=[RATE_LO, RATE_HI],
               requests_per_scale={str(s): len(sub) for s, (_, sub) in per.items()}, runs=a.runs, warmup=a.warmup)
    for m in ways:
        res[m] = dict(phase1_batches=counts[m][0], phase2_batches=counts[m][1], control_batches=counts[m][2],
                      wall_ms_median=round(statistics.median(wall[m]), 2), wall_ms_min=round(min(wall[m]), 2),
                      wall_ms_max=round(max(wall[m]), 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--mode", choices=("both", "all", "plain", "ragged", "ragged_ref", "ragged_frames", "ragged_decoder",
                                       "controls"), default="both")
    ap.add_argument("--engine", choices=("default", "precise"), default="default",
                    help="the engine under the schedulers: the bf16 default, or StyleTTSZS(precise=True)")
    ap.add_argument("--ref-s", default=None, metavar="LO,HI",
                    help="reference lengths seeded uniformly in [LO, HI] seconds (default: 3 s for every request)")
    a = ap.parse_args()
    ref_s = None
    if a.ref_s is not None:
        ref_s = tuple(float(v) for v in a.ref_s.split(","))
        if len(ref_s) != 2 or not 0 < ref_s[0] <= ref_s[1]:
            raise SystemExit("--ref-s takes LO,HI in seconds, 0 < LO <= HI")
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.scheduler import BucketScheduler
    from stzs.spec import SPEC_V0 as S
    if not torch.cuda.is_available():
        raise SystemExit("ragged_traffic.py measures on the GPU: none is visible")
    eng = StyleTTSZS(S, init_params(S, seed=0), device="cuda:0", precise=a.engine == "precise")
    reqs = make_requests(S, a.requests, ref_s=ref_s)
    if a.mode == "controls":
        print(json.dumps(controls_mode(a, eng, S, reqs)))
        return
    # (ragged_text, ragged_ref, ragged_frames, ragged_decoder)
    modes = {"plain": (False, False, False, False), "ragged": (True, False, False, False),
             "ragged_ref": (True, True, False, False), "ragged_frames": (True, True, True, False),
             "ragged_decoder": (True, True, True, True)}
    if a.mode == "both":
        modes = {m: modes[m] for m in ("plain", "ragged")}
    elif a.mode != "all":
        modes = {a.mode: modes[a.mode]}
    sch = {m: BucketScheduler(eng, max_batch=a.max_batch, steps=STEPS, cfg_scale=CFG, ragged_text=rt, ragged_ref=rr,
                              ragged_frames=rf, ragged_decoder=rd)
           for m, (rt, rr, rf, rd) in modes.items()}
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
    res = dict(engine=a.engine, requests=a.requests, tokens=[int(r.tokens.shape[0]) for r in reqs], steps=STEPS, cfg=CFG,
               ref_s=REF_S if ref_s is None else list(ref_s), runs=a.runs, warmup=a.warmup)
    if ref_s is not None:
        res["ref_samples"] = [int(r.ref_wav.shape[0]) for r in reqs]
    for m in sch:
        st = sch[m].stats
        res[m] = dict(phase1_batches=st["phase1_batches"], phase2_batches=st["phase2_batches"],
                      wall_ms_median=round(statistics.median(wall[m]), 2), wall_ms_min=round(min(wall[m]), 2),
                      wall_ms_max=round(max(wall[m]), 2), phase1_ms_median=round(statistics.median(ph1[m]), 2),
                      phase1_ms_min=round(min(ph1[m]), 2), phase1_ms_max=round(max(ph1[m]), 2),
                      ref_pad_share=round(st["ref_pad_share"], 4), prosody_batches=st["prosody_batches"],
                      frame_pad_share=round(st["frame_pad_share"], 4), decoder_batches=st["decoder_batches"],
                      decoder_pad_share=round(st["decoder_pad_share"], 4))
    if "plain" in sch:  # every schedule computed the same waveforms
        for m in sch:
            if m != "plain":
                worst = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(outs[m], outs["plain"]))
                res[f"max_rel_diff_{m}_vs_plain"] = worst
    print(json.dumps(res))


if __name__ == "__main__":
    main()
