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

    python tools/ragged_traffic.py [--requests 64] [--runs 7] [--warmup 2] [--ref-s LO,HI]
                                   [--mode both|all|plain|ragged|ragged_ref|ragged_frames|ragged_decoder]

--mode both: plain and ragged (the measurement of "Ragged text batches"); all: the five schedules.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--mode", choices=("both", "all", "plain", "ragged", "ragged_ref", "ragged_frames", "ragged_decoder"),
                    default="both")
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
    eng = StyleTTSZS(S, init_params(S, seed=0), device="cuda:0")
    reqs = make_requests(S, a.requests, ref_s=ref_s)
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
    res = dict(requests=a.requests, tokens=[int(r.tokens.shape[0]) for r in reqs], steps=STEPS, cfg=CFG,
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
