"""Call history of one engine (a plain helper module, like refops.py): the engine caches ONE storage per (key, dtype)
(StyleTTSZS.buf), zeroes a zero=True buffer when it is allocated and whenever its requested shape changes, and at no
other time -- so a call at a shape the engine has already seen runs over whatever the earlier calls left there.  The
contract: padding columns of act() buffers stay zero (the engine's own invariant), data regions are
finite and unspecified between calls, a zero=False buffer promises nothing.  Under that contract the result of a
top-level call must be the bits a fresh engine gives.

    track(eng)        wraps eng.buf / eng.act (and eng.decode, to keep the stage trace of the last call) ON THE
                      INSTANCE: per cache entry the zero flag of the last request and, for act() buffers, (B, T, C)
    dirty(eng)        every tracked storage into a state the contract allows and a fresh engine never has; only ever
                      between top-level calls
    fresh(eng, call)  the call on a twin (same packed weights, empty cache), host copies, once per call
    first_diff(...)   the failure message: call, predecessor, first differing row / sample / 40-fps frame / stage

What dirty() writes, per kind (classify()):
    "nan"   zero=False floating-point buffers: NaN over the whole storage capacity
    "act"   act() buffers: the data columns [0, C) of the current view <- 1000.0 (bf16 / fp32; exact in bf16) or 256.0
            (fp8) -- moderate on purpose, a statistics pass over it cannot overflow; the padding columns are left alone
    "keep"  other zero=True float buffers (gen.har, gen.har_w, gen.post_w, dec.F0w, dec.Nw): as the last call left them
    "int"   integer / byte buffers (lengths, indices, LSTM exchange and sync words): NEVER touched -- a garbage index or
            sync word could send a kernel out of range or make it wait for ever; they go stale through real calls only
    "pool"  the non-tuple keys of eng._bufs (scratch slabs, split-K / tile counters): never touched; nor is eng._consts

The calls of tests/test_gpu_engine_history.py and tests/test_engine_history_host.py are built here too (make_calls)."""
import torch

FILL = {torch.float32: 1000.0, torch.bfloat16: 1000.0, torch.float16: 1000.0, torch.float8_e4m3fn: 256.0}
_F8 = (torch.float8_e4m3fn,)
_F8_NAN, _F8_256 = 0x7F, 0x78  # e4m3fn: S.1111.111 is NaN; 2^8 = exponent field 15, mantissa 0
_WRAPPED = ("buf", "act", "decode", "_history", "_history_name", "_last_trace")


def _rup8(c):
    return (c + 7) // 8 * 8


def track(eng, name=None):
    """wrap eng.buf / eng.act / eng.decode on the instance (the class is left alone) -> the record
    {(key, dtype): dict(zero=bool, act=(B, T, C) | None)}, updated by every request.  Idempotent."""
    if "_history" in eng.__dict__:
        return eng._history
    cls = type(eng)
    hist = eng._history = {}
    eng._history_name = name or getattr(eng, "_history_name", "engine")
    eng._last_trace = None
    pending = []

    def buf(key, shape, dtype=torch.bfloat16, zero=False):
        out = cls.buf(eng, key, shape, dtype, zero)
        hist[(key, dtype)] = dict(zero=bool(zero), act=pending.pop() if pending else None)
        return out

    def act(key, B, T, C, dtype=torch.bfloat16):
        pending.append((int(B), int(T), int(C)))
        try:
            return cls.act(eng, key, B, T, C, dtype)
        finally:
            del pending[:]

    def decode(pro, codes, seeds, istft=True, frame_lens=None, trace=None, rows=None):
        # (the trace only collects references to the stages' buffers: no launch is added)
        tr = eng._last_trace = {} if trace is None else trace
        return cls.decode(eng, pro, codes, seeds, istft=istft, frame_lens=frame_lens, trace=tr, rows=rows)

    eng.buf, eng.act, eng.decode = buf, act, decode
    return hist


def twin(eng):
    """eng.twin() with wrappers of its own (twin() copies the instance dictionary, the wrappers with it -- they
    would send the twin's requests to eng's cache)"""
    t = eng.twin()
    name = getattr(eng, "_history_name", None)
    for k in _WRAPPED:
        t.__dict__.pop(k, None)
    track(t, name)
    return t


def classify(eng):
    """-> {key of eng._bufs: "nan" | "act" | "keep" | "int" | "pool"}; a tuple key track() never saw is an error"""
    out = {}
    for k, ent in eng._bufs.items():
        if not isinstance(k, tuple):
            out[k] = "pool"
            continue
        rec = eng._history.get(k)
        assert rec is not None, f"buffer {k} was requested before track()"
        dt = ent[0].dtype
        if not dt.is_floating_point:
            out[k] = "int"
        elif not rec["zero"]:
            out[k] = "nan"
        elif rec["act"] is not None:
            out[k] = "act"
        else:
            out[k] = "keep"
    return out


def dirty(eng):
    """poison the engine's cached buffers within the buffer contract (module docstring) -> classify(eng).  Between
    top-level calls only: never between stages that hand results to each other through engine buffers."""
    kinds = classify(eng)
    for k, kind in kinds.items():
        if kind == "nan":
            store = eng._bufs[k][0]
            if store.dtype in _F8:
                store.view(torch.uint8).fill_(_F8_NAN)
            else:
                store.fill_(float("nan"))
        elif kind == "act":
            view = eng._bufs[k][2]
            B, T, C = eng._history[k]["act"]
            assert tuple(view.shape) == (B, T, _rup8(C)), (k, tuple(view.shape), (B, T, C))
            if view.dtype in _F8:
                view.view(torch.uint8)[:, :, :C] = _F8_256
            else:
                view[:, :, :C] = FILL[view.dtype]
    return kinds


# ---- the calls -------------------------------------------------------------------------------------------------------

T = 12
FRAMES_A = [7, 1, 3, 6]
FRAMES_B = [1, 7, 6, 3]   # long where FRAMES_A is short, short where it is long
TEXT_LENS = [12, 5, 9, 3]
SEEDS = [3, 4, 5, 6]
STEPS, CFG = 2, 5.0
CHUNK, HALO = 2, 1        # 7 frames in chunks of 2: four chunks, the last of one frame
SCALES = [5.0, 1.0, 2.5, 0.0]
RATES = [4.0, 2.0, 1.7, 3.0]   # fast rates: the predicted frame counts stay small
SHIFTS = [0.0, 12.0, -7.0, 3.5]
REF_SR, OUT_SR = 16000, 22050


def _split(n, T=T):
    return [n // T + (1 if t < n % T else 0) for t in range(T)]


class Call:
    """one top-level call: fn(eng) -> (wav, frame_lens | None) for synth, an iterator of (first sample, chunk) for a
    stream; run() makes it and returns host copies"""

    def __init__(self, name, fn, stream=False, abandon=False, out_sr=None):
        self.name, self.fn, self.stream, self.abandon, self.out_sr = name, fn, stream, abandon, out_sr

    def __repr__(self):
        return self.name


class Calls(dict):
    """{name: Call}; .data: the host inputs they share (tok, ref, eps, dur7: 7 frames per row)"""
    data = None


def make_calls(S, B=4, T=T, check=True):
    """the inputs (built once, seed 31: those of tests/test_gpu_ragged_stream_stages.py at B = 4) and the calls of the
    table in tests/test_gpu_engine_history.py -> {name: Call}.  B < 4: the uniform subset on the first B rows.
    check: synth()'s own status check (False on "cpu": it asks the runtime whether a graph is being captured)."""
    g = torch.Generator().manual_seed(31)
    tok = torch.randint(1, S.n_symbols, (4, T), generator=g)[:B]
    N = S.sr // 2
    ref = (torch.randn(4, N, generator=g) * 0.1)[:B]
    eps = torch.randn(4, S.L_s, S.code_dim, generator=g)[:B]
    ref16 = (torch.randn(4, N * REF_SR // S.sr, generator=g) * 0.1)[:B]
    kw = dict(steps=STEPS, cfg_scale=CFG, noise=eps, seeds=SEEDS[:B], check=check)
    chunk_s = CHUNK * S.frame40 / S.sr

    def uni(n):
        return torch.tensor([_split(n, T)] * B, dtype=torch.int32)

    calls = Calls()
    calls.data = dict(tok=tok, ref=ref, eps=eps, dur7=uni(7))

    def add(name, fn, **k):
        calls[name] = Call(name, fn, **k)

    add("U", lambda e: (e.synth(tok, ref, durations=uni(7), **kw)["wav"], None))
    add("U2", lambda e: (e.synth(tok, 2 * ref, durations=uni(7), **dict(kw, noise=2 * eps))["wav"], None))
    add("Us", lambda e: (e.synth(tok[:, :8], ref, durations=torch.tensor([_split(5, 8)] * B, dtype=torch.int32),
                                 **kw)["wav"], None))   # a smaller shape: 8 tokens, 5 frames
    add("Ul", lambda e: (e.synth(tok, ref, durations=uni(9), **kw)["wav"], None))   # a larger one: 9 frames
    add("Sw", lambda e: e.synth_stream(tok, ref, durations=uni(7), chunk_s=chunk_s, **kw), stream=True)
    # (the uniform chunked decoder: for tests/test_engine_history_host.py -- the ragged one reads device lengths back)
    add("Scu", lambda e: e.synth_stream(tok, ref, durations=uni(7), chunk_s=chunk_s, chunked_halo=HALO, **kw),
        stream=True)
    if B < 4:
        return calls
    rl = [N, 7 * N // 10 + 1, N, S.mel_nfft // 2 + 1]
    n16 = ref16.shape[1]
    rl16 = [n16, 7 * n16 // 10 + 1, n16, 700]   # 700 samples at 16 kHz: 1050 at 24 kHz, just above mel_nfft / 2 + 1

    def rag(frames, tl=None):
        d = torch.zeros(B, T, dtype=torch.int32)
        for b, n in enumerate(frames):
            w = T if tl is None else tl[b]
            d[b, :w] = torch.tensor(_split(n, w), dtype=torch.int32)
        return d

    add("Rt", lambda e: (e.synth(tok, ref, durations=rag([7] * B, TEXT_LENS), text_lens=TEXT_LENS, ref_lens=rl,
                                 **kw)["wav"], None))
    add("Ra", lambda e: e.synth(tok, ref, durations=rag(FRAMES_A), ragged_frames=True, **kw))
    add("Rb", lambda e: e.synth(tok, ref, durations=rag(FRAMES_B), ragged_frames=True, **kw))
    add("Rp", lambda e: e.synth(tok, ref, text_lens=TEXT_LENS, ref_lens=rl, ragged_frames=True, **kw))
    add("C", lambda e: e.synth(tok, ref, steps=STEPS, noise=eps, seeds=SEEDS, ragged_frames=True, check=check,
                               controls=e.row_controls(B, cfg_scale=SCALES, speed=RATES, pitch_shift=SHIFTS)))
    add("Sr", lambda e: e.synth_stream(tok, ref, durations=rag(FRAMES_A), chunk_s=chunk_s, ragged_frames=True, **kw),
        stream=True)
    add("Sc", lambda e: e.synth_stream(tok, ref, durations=rag(FRAMES_A), chunk_s=chunk_s, chunked_halo=HALO,
                                       ragged_frames=True, **kw), stream=True)
    add("X", lambda e: e.synth(tok, ref16, durations=rag(FRAMES_A), ragged_frames=True, ref_sr=REF_SR, ref_lens=rl16,
                               out_sr=OUT_SR, out_dtype=torch.int16, **kw), out_sr=OUT_SR)
    add("A", calls["Sr"].fn, stream=True, abandon=True)
    return calls


def _host(t):
    return t.detach().cpu().clone()


def host_trace(eng):
    """host copies of the logical channels of the last decode()'s traced stages (its buffers are reused by the next
    call), or {} where the call made no whole-decoder decode()"""
    tr = eng._last_trace or {}
    return {k: _host(v.t[:, :, v.c0:v.c0 + v.C]) for k, v in tr.items()}


def run(eng, call, check=True):
    """make the call -> dict(wav, fl (list | None), spans (list | None), har (host tensor | None)); an abandoned
    stream -> None.  check: the LSTM status word must be 0 afterwards (a timed-out exchange here would be a sync word
    this module disturbed)."""
    eng._last_trace = None
    if call.abandon:
        it = call.fn(eng)
        next(it)
        it.close()
        res = None
    elif call.stream:
        eng.frame_lens = None
        parts, spans, end = [], [], 0
        for n0, w in call.fn(eng):
            assert n0 == end, (call.name, n0, end)
            end = n0 + w.shape[1]
            spans.append((n0, w.shape[1]))
            parts.append(w.clone())
        fl = None if eng.frame_lens is None else _host(eng.frame_lens).tolist()
        res = dict(wav=_host(torch.cat(parts, 1)), fl=fl, spans=spans)
    else:
        wav, fl = call.fn(eng)
        res = dict(wav=_host(wav), fl=None if fl is None else _host(fl).tolist(), spans=None)
    if res is not None:
        tr = eng._last_trace or {}
        res["har"] = _host(tr["har"].t[:, :, :tr["har"].C]) if "har" in tr else None
    if check:
        assert eng.check_status() == 0, f"{call.name}: LSTM exchange timed out"
    return res


_FRESH = {}


def fresh(eng, call):
    """the call on a twin of eng -- the same packed weights, an empty buffer cache -> run()'s dict with the host
    trace under "trace"; computed once per (engine, call) and never changed afterwards"""
    key = (getattr(eng, "_history_name", None), id(eng.W), call.name)
    if key not in _FRESH:
        t = twin(eng)
        res = run(t, call)
        if res is not None:
            res["trace"] = host_trace(t)
        _FRESH[key] = res
    return _FRESH[key]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def trace_rows(S, n):
    """valid rows of every traced decoder stage for a row of n 40-fps frames (two generator stages)"""
    r0, r1 = S.up_rates
    return dict(gen_in=2 * n, har=2 * n * S.hop // S.istft_hop + 1, mrf_in0=2 * n * r0, mrf_out0=2 * n * r0,
                mrf_in1=2 * n * r0 * r1 + 1, mrf_out1=2 * n * r0 * r1 + 1, post=2 * n * r0 * r1 + 1)


def first_stage_diff(S, got, want, fl):
    """the first traced stage (in decoder order) whose valid rows differ -> text, or None"""
    for k in ("gen_in", "har", "mrf_in0", "mrf_out0", "mrf_in1", "mrf_out1", "post"):
        if k not in got or k not in want:
            continue
        a, b = got[k], want[k]
        if a.shape != b.shape:
            return f"stage {k}: shapes {tuple(a.shape)} / {tuple(b.shape)}"
        for row in range(a.shape[0]):
            n = a.shape[1] if fl is None else min(a.shape[1], trace_rows(S, fl[row])[k])
            ne = (_bits(a[row, :n]) != _bits(b[row, :n])).flatten(1).any(1) if n else torch.zeros(0, dtype=torch.bool)
            if bool(ne.any()):
                return f"stage {k}: row {row} differs first at its row {int(ne.nonzero()[0])} of {n} valid"
    return None


def first_diff(a, b, frame40, call="", pred="", stage=None):
    """two waveforms [B, n] that should be equal -> the failure message: the call, what ran before it, the first
    differing row, sample and 40-fps frame (frame40 samples each), the count, and `stage` (first_stage_diff)"""
    head = f"call {call} after {pred or 'nothing'}"
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"{head}: got {tuple(a.shape)} {a.dtype}, a fresh engine gives {tuple(b.shape)} {b.dtype}"
    ne = a != b
    if a.is_floating_point():
        ne |= torch.isnan(a) != torch.isnan(b)
    if not bool(ne.any()):
        return f"{head}: equal"
    row, n = (int(v) for v in ne.nonzero()[0])
    msg = (f"{head}: differs from a fresh engine in {int(ne.sum())} of {ne.numel()} samples, first at row {row} "
           f"sample {n} (40-fps frame {n // max(int(frame40), 1)}): {a[row, n].item()!r} / {b[row, n].item()!r}")
    return msg + (f"; {stage}" if stage else "")
