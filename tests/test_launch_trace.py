"""Host-side determinism of the engine (tools/launch_trace.py): with the library replaced by a recording stub, the
ordered list of library calls -- every argument struct, workspace query and buffer key -- that a synthesis enqueues
is a function of the engine's configuration and the input shapes alone.  No device is touched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_launch_trace_deterministic():
    """the eight cases (bf16 sequential / trio MRF, precise, fp8, precise + fp8, the latency tables, the streaming and
    the chunked decoder) at the tiny spec, twice on fresh engines: identical traces, and every case launches."""
    import launch_trace as T
    import torch
    from stzs import _lib, engine

    saved = (_lib.load, engine.StyleTTSZS.stream, torch.from_numpy)
    first, second = T.run_cases("tiny"), T.run_cases("tiny")
    assert (_lib.load, engine.StyleTTSZS.stream, torch.from_numpy) == saved  # (the stub is gone again)
    assert [n for n, _, _ in first] == ["bf16.b5", "bf16.b2", "precise.b2", "fp8.b1", "precise+fp8.b1", "latency.b1",
                                        "stream.b2", "chunked.b1"]
    for (name, calls, launches), (name2, calls2, launches2) in zip(first, second):
        assert name == name2 and launches == launches2 and launches > 0, (name, launches, launches2)
        assert len(calls) > launches // 2, name
        assert T.digest(calls) == T.digest(calls2), name
        assert calls == calls2, name
    # the two MRF schedules and the batch-1 tables really are different launch sequences
    assert len({T.digest(c) for _, c, _ in first}) == len(first)
