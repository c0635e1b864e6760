"""Host-side launch trace (the CPU counterpart of tools/synth_hash.py): every library call a synthesis enqueues, in
order, with every argument -- recorded WITHOUT a device.  stzs._lib.load is replaced by a recording stub and
StyleTTSZS.stream is overridden, so the engines pack and enqueue on device "cpu" and nothing is launched.  Two trees
whose dumps are equal enqueue the same launches with the same argument structs: the check for a host refactor.

    python tools/launch_trace.py --spec v0 --dump a.jsonl      # one line per case: name, calls, launches, sha256

Recorded per call: the function name and per argument the struct's fields (pointer fields as null / ptr; an optional
pointer of type stzs._lib.opt_vp only when it is set, so a new optional field leaves the digests alone), the elements
of a struct array, or the scalar (integers >= 2^24 are addresses: "ptr"); each case ends with one "buffers" record,
the engine's buffer and scratch keys in the order they were first requested.  Stub results: *_workspace queries a fixed
size, stzs_conv1d_group its count, stzs_istft_stream_span a fixed arithmetic span, everything else 0.

Three things beyond a plain call recorder, all this tool's own choices: the closing "buffers" record (so a change in
the order of first requests shows up); torch.from_numpy is replaced by a copying version while the cases run, and put
back afterwards (on "cpu" an uploaded host constant would alias its numpy array, whose alignment varies from run to
run, and the engine routes on 16- / 32-byte alignment -- a process-wide patch, so nothing else should use torch
concurrently); and the chunked case runs at chunk_s = 0.25 (20 windows) to keep its trace short, the streaming case at
0.05.  Importing the module puts the repository root and the package directory on sys.path, like the other tools.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "styletts-zs_amd")]
import torch  # noqa: E402

from bench import CFG, make_inputs  # noqa: E402
from stzs import _lib, engine  # noqa: E402
from stzs.params import init_params  # noqa: E402
from stzs.spec import SPEC_TINY, SPEC_V0  # noqa: E402

WORKSPACE_BYTES = 1 << 20
_BYREF = type(C.byref(C.c_int()))


def _scalar(v):
    if isinstance(v, float):
        return v
    return "ptr" if isinstance(v, int) and abs(v) >= 1 << 24 else v


def _struct(s):
    out = {}
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is getattr(_lib, "opt_vp", None):  # an optional pointer: recorded when set (NULL: the call without it)
            if v.value:
                out[name] = "ptr"
            continue
        out[name] = ("ptr" if v else "null") if typ is C.c_void_p else _scalar(v)
    return out


def _arg(v):
    if isinstance(v, _BYREF):
        v = v._obj
    if isinstance(v, C.Structure):
        return _struct(v)
    if isinstance(v, C.Array):
        return [_struct(e) for e in v]
    if isinstance(v, C.c_void_p):
        return "ptr" if v.value else "null"
    if isinstance(v, C._SimpleCData):  # (an output slot: stzs_istft_stream_span's n0 / n1)
        return "out"
    return "null" if v is None else _scalar(v)


class RecordingLib:
    """stands in for the loaded library: records each call into .calls and returns the stub result"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("stzs_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append([name] + [_arg(a) for a in args])
            if name.endswith("_workspace"):
                return WORKSPACE_BYTES
            if name == "stzs_conv1d_group":
                return args[1]
            if name == "stzs_istft_stream_span":  # (f0, Fc, final, n_fft, hop, &n0, &n1) -> carried frames
                f0, Fc, fin, _, hop, n0, n1 = args
                n0._obj.value, n1._obj.value = f0 * hop, (f0 + Fc - (1 if fin else 0)) * hop
                return 3
            if name == "stzs_strerror":
                return b"stub"
            return 0
        return fn


class _Patched:
    """the stub in place of stzs._lib.load (unless record is false: tools/dispatch_trace.py keeps the real load, of a
    library linked against a recording runtime), and a null stream for every engine, while the cases run"""

    def __init__(self, record=True):
        self.lib = RecordingLib() if record else None

    def __enter__(self):
        self.saved = (_lib.load, engine.StyleTTSZS.stream, torch.from_numpy)
        if self.lib:
            _lib.load = lambda: self.lib
        engine.StyleTTSZS.stream = lambda eng: C.c_void_p(0)
        # on "cpu" an uploaded host constant would alias its numpy array, whose alignment varies from run to run (the
        # engine routes on 16- and 32-byte alignment); a copy gives it torch's 64-byte alignment, as a device upload
        from_numpy = torch.from_numpy
        torch.from_numpy = lambda arr: from_numpy(arr).clone()
        return self.lib

    def __exit__(self, *exc):
        _lib.load, engine.StyleTTSZS.stream, torch.from_numpy = self.saved


def run_cases(spec_name="tiny", record=True, on_case=None):
    """-> [(case name, [call, ...], engine.launches)] of the eight cases on fresh engines; record = False keeps the
    real stzs._lib.load (no calls recorded), on_case(name) is called before each case's synthesis"""
    S = {"tiny": SPEC_TINY, "v0": SPEC_V0}[spec_name]
    P = init_params(S, 0)
    out = []
    with _Patched(record) as lib:
        mk = lambda **kw: engine.StyleTTSZS(S, P, device="cpu", **kw)
        bf16, pf8 = mk(), mk(precise=True, fp8_denoiser=True)
        lat = engine.StyleTTSZS(S, None, device="cpu", packed=bf16.W, dn_splitk=engine.LATENCY_DN_SPLITK,
                                dn_rows=engine.LATENCY_DN_ROWS, te_splitk=engine.LATENCY_TE_SPLITK,
                                blk_splitk=engine.LATENCY_BLK_SPLITK, branch_streams=False)
        cases = [("bf16.b5", bf16, 5, 2, None), ("bf16.b2", bf16.twin(), 2, 2, None),
                 ("precise.b2", mk(precise=True), 2, 2, None), ("fp8.b1", mk(fp8_denoiser=True), 1, 2, None),
                 ("precise+fp8.b1", pf8, 1, 2, None), ("latency.b1", lat, 1, 10, None),
                 ("stream.b2", bf16.twin(), 2, 2, dict(chunk_s=0.05)),
                 ("chunked.b1", pf8.twin(), 1, 2, dict(chunk_s=0.25, chunked_halo=2))]
        for name, eng, B, steps, stream in cases:
            tok, ref, eps, dur = make_inputs(S, B, 7)
            kw = dict(steps=steps, cfg_scale=CFG, noise=eps, durations=dur, seeds=list(range(B)),
                      n_frames=int(dur.sum(1).max()), check=False)
            calls = lib.calls if lib else []
            del calls[:]
            if on_case:
                on_case(name)
            if stream is None:
                eng.synth(tok, ref, **kw)
            else:
                for _ in eng.synth_stream(tok, ref, **kw, **stream):
                    pass
            # (last record: the buffer / scratch keys in the order they were first requested)
            out.append((name, calls + [["buffers"] + [str(k) for k in eng._bufs]], eng.launches))
    return out


def digest(calls):
    return hashlib.sha256("\n".join(json.dumps(c) for c in calls).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--spec", choices=("tiny", "v0"), default="tiny")
    ap.add_argument("--dump", metavar="FILE", help="write the full trace as JSON lines")
    args = ap.parse_args()
    res = run_cases(args.spec)
    for name, calls, launches in res:
        print(f"{name:15s} calls={len(calls):5d} launches={launches:5d} sha256={digest(calls)}")
    if args.dump:
        with open(args.dump, "w") as f:
            for name, calls, launches in res:
                f.write(json.dumps(dict(case=name, calls=len(calls), launches=launches)) + "\n")
                for c in calls:
                    f.write(json.dumps(c) + "\n")


if __name__ == "__main__":
    main()
