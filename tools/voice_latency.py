"""Batch-1 synth() from a reference clip against synth() from an enrolled voice: the configs[1] shape
(v0 dims, 10-step CFG 5, bench.py's latency engine and inputs), each captured into one graph; the two graphs are
replayed alternately, WARM pairs untimed, then N timed pairs, each replay between two device synchronisations.

    python tools/voice_latency.py            # N=300 WARM=20 by default (env N, WARM)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "styletts-zs_amd")]
import torch  # noqa: E402

from bench import CFG, STEPS_LATENCY, make_inputs  # noqa: E402
from stzs.engine import StyleTTSZS, latency_engine  # noqa: E402
from stzs.params import init_params  # noqa: E402
from stzs.spec import SPEC_V0 as S  # noqa: E402
from stzs.voice import VoiceBank  # noqa: E402

base = StyleTTSZS(S, init_params(S, 0), device="cuda:0")
tok, ref, eps, dur = (t.cuda() for t in make_inputs(S, 1, 1000))
nf = int(dur[0].sum())
kw = dict(steps=STEPS_LATENCY, cfg_scale=CFG, noise=eps, durations=dur, seeds=[7], n_frames=nf)
engines = {"ref_wav": latency_engine(S, base.W), "voices": latency_engine(S, base.W)}  # (a buffer cache per graph)
bank = VoiceBank(engines["voices"], 1)
rows = engines["voices"].voice_rows(1, bank, [bank.add(engines["voices"].enroll(ref[0]))])
calls = {"ref_wav": lambda: engines["ref_wav"].synth(tok, ref, **kw),
         "voices": lambda: engines["voices"].synth(tok, None, voices=rows, **kw)}
graphs, wavs, launches = {}, {}, {}
for k, fn in calls.items():
    n0 = engines[k].launches
    fn()
    launches[k] = engines[k].launches - n0
    graphs[k], out = engines[k].capture(fn)
    graphs[k].replay()
    torch.cuda.synchronize()
    wavs[k] = out["wav"].clone()
assert torch.equal(wavs["ref_wav"], wavs["voices"]), "the two paths must give the same waveform"
n, warm = int(os.environ.get("N", 300)), int(os.environ.get("WARM", 20))
ts = {k: [] for k in calls}
for i in range(warm + n):
    for k in calls:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        graphs[k].replay()
        torch.cuda.synchronize()
        if i >= warm:
            ts[k].append((time.perf_counter() - t0) * 1e3)
for k, v in ts.items():
    v.sort()
    print(f"{k:8s} launches/synth {launches[k]:4d}  p50 {v[len(v) // 2]:.3f} ms  p10 {v[len(v) // 10]:.3f}  "
          f"p90 {v[9 * len(v) // 10]:.3f}  min {v[0]:.3f}  ({n} replays, alternated, {warm} warm-up pairs)")
