"""Enrolled voices: encode a reference once, synthesise from it per row.

    v = eng.enroll(clip)                          # Voice: pre-quantiser prompt features + their discrete codes
    bank = VoiceBank(eng, capacity=16)
    i = bank.add(v)                               # device-resident, fixed addresses
    rows = eng.voice_rows(B, bank, [i] * B)       # VoiceRows: device arrays of ids / weights / counts
    out = eng.synth(tokens, None, voices=rows, ...)

A Voice holds z fp32 [L_s, code] and idx int32 [L_s, G] on the engine's device.  Indices only mean something under the
codebook that made them, so every voice carries the fingerprint of the prompt front end it came from (a hash of the
packed pe.* parameters, codebook included, and of the spec fields that front end reads); a bank refuses a voice whose
fingerprint is not its engine's.

VoiceRows is modelled on RowControls: the object owns the device arrays src int32 [B, Kmax], w fp32 [B, Kmax] and cnt
int32 [B] that stzs_voice_prompt reads; what is launched -- the gather form when every row is one voice, else the mix
form at that Kmax -- is fixed when the object is made, and set() rewrites the arrays in place (a captured graph replays
for other speakers), raising ValueError for a structural change.
"""
from __future__ import annotations

import hashlib
import json
import math
import operator
from typing import List, Optional, Sequence

import torch

KMAX = 8  # include/stzs.h: stzs_voice_prompt takes at most 8 sources per row
FORMAT = "stzs-voices-v0"
# the spec fields the prompt front end reads (log-mel geometry, encoder widths, the quantiser's shape)
FP_FIELDS = ("sr", "hop", "mel_nfft", "mel_win", "n_mels", "pe_ch", "L_s", "code_dim", "vq_group", "vq_size")
# arena entries left out of the fingerprint: the precise front end's split streams, derived from the same parameters
# (a voice enrolled on either front end is valid on the other: the codebook is one)
_FP_SKIP = (".wx3", ".wfx3", ".w32")


def engine_fingerprint(eng) -> str:
    """sha256 over the spec fields of FP_FIELDS and the bytes of every packed pe.* arena entry (convs, projection,
    biases, the fp32 codebook).  Read back from the device once per packed model and kept on it."""
    W = eng.W
    fp = getattr(W, "_voice_fingerprint", None)
    if fp is None:
        h = hashlib.sha256()
        h.update(json.dumps({k: getattr(eng.spec, k) for k in FP_FIELDS}, sort_keys=True).encode())
        for k in sorted(W.arena.views):
            if k.startswith("pe.") and not k.endswith(_FP_SKIP):
                h.update(k.encode())
                h.update(W.arena.views[k].detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
        fp = W._voice_fingerprint = h.hexdigest()
    return fp


def normalise_weights(weights, n: int, what: str = "weights") -> List[float]:
    """n source weights -> the float32 values w_k = float32(weights_k / sum(weights)), the division in float64 on the
    host (None: equal weights).  One source gives exactly 1.0.  ValueError for a wrong count, a non-finite or negative
    weight, a zero sum."""
    if n < 1:
        raise ValueError(f"{what}: at least one source is needed")
    if weights is None:
        ws = [1.0] * n
    else:
        try:
            ws = [float(v) for v in weights]
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what} must be {n} numbers: {e}")
    if len(ws) != n:
        raise ValueError(f"{what}: {len(ws)} weights for {n} sources")
    if any(not math.isfinite(v) or v < 0.0 for v in ws):
        raise ValueError(f"{what} must be finite and >= 0, got {ws}")
    tot = math.fsum(ws)
    if tot <= 0.0:
        raise ValueError(f"{what} must not sum to zero, got {ws}")
    return torch.tensor([v / tot for v in ws], dtype=torch.float64).to(torch.float32).tolist()


class Voice:
    """one enrolled voice: z fp32 [L_s, code] (the pre-quantiser prompt features, for blending) and idx int32 [L_s, G]
    (their discrete codes, for the gather form) on the engine's device, the fingerprint of the engine that made it, the
    number of clips it was built from and the front end that ran ("bf16" | "precise")."""

    def __init__(self, z: torch.Tensor, idx: torch.Tensor, fingerprint: str, clips: int = 1, frontend: str = "bf16"):
        if z.dim() != 2 or idx.dim() != 2 or z.shape[0] != idx.shape[0]:
            raise ValueError(f"Voice: z [L, code] and idx [L, G] expected, got {tuple(z.shape)} {tuple(idx.shape)}")
        if z.dtype != torch.float32 or idx.dtype != torch.int32:
            raise ValueError(f"Voice: z fp32 and idx int32 expected, got {z.dtype} {idx.dtype}")
        if frontend not in ("bf16", "precise"):
            raise ValueError(f"Voice: frontend must be 'bf16' or 'precise', got {frontend!r}")
        self.z, self.idx = z.contiguous(), idx.contiguous()
        self.fingerprint, self.clips, self.frontend = str(fingerprint), int(clips), frontend

    def __repr__(self):
        return (f"Voice(L={self.z.shape[0]}, code={self.z.shape[1]}, clips={self.clips}, frontend={self.frontend!r}, "
                f"fingerprint={self.fingerprint[:12]}...)")


def _check_voice(voice, eng, what: str):
    S = eng.spec
    if not isinstance(voice, Voice):
        raise ValueError(f"{what}: a Voice is expected, got {type(voice).__name__}")
    if voice.fingerprint != engine_fingerprint(eng):
        raise ValueError(f"{what}: the voice was enrolled under another prompt encoder / codebook (fingerprint "
                         f"{voice.fingerprint[:12]}..., the engine's is {engine_fingerprint(eng)[:12]}...)")
    G = S.code_dim // S.vq_group
    if tuple(voice.z.shape) != (S.L_s, S.code_dim) or tuple(voice.idx.shape) != (S.L_s, G):
        raise ValueError(f"{what}: voice shapes {tuple(voice.z.shape)} {tuple(voice.idx.shape)} do not fit the spec")


class VoiceBank:
    """`capacity` voices resident on the engine's device: z fp32 [capacity, L_s, code] and idx int32 [capacity, L_s, G],
    allocated once -- add() and replace() write in place, so the addresses a captured graph holds stay valid and a
    replay after replace(id, v2) sees v2.  Slots not yet added hold zeros (a valid voice as far as the kernel's bounds
    go; VoiceRows refuses their ids on the host)."""

    def __init__(self, engine, capacity: int):
        S = engine.spec
        if int(capacity) < 1:
            raise ValueError(f"VoiceBank: capacity must be >= 1, got {capacity}")
        self.eng, self.capacity = engine, int(capacity)
        G = S.code_dim // S.vq_group
        self.z = torch.zeros(self.capacity, S.L_s, S.code_dim, dtype=torch.float32, device=engine.device)
        self.idx = torch.zeros(self.capacity, S.L_s, G, dtype=torch.int32, device=engine.device)
        self.meta = []  # per added voice: dict(clips, frontend)

    def __len__(self):
        return len(self.meta)

    @property
    def fingerprint(self) -> str:
        return engine_fingerprint(self.eng)

    def _write(self, i: int, voice: Voice):
        self.z[i].copy_(voice.z)
        self.idx[i].copy_(voice.idx)

    def add(self, voice: Voice) -> int:
        """-> the voice's id.  ValueError for a fingerprint that is not the engine's, and when the bank is full."""
        _check_voice(voice, self.eng, "VoiceBank.add")
        if len(self.meta) >= self.capacity:
            raise ValueError(f"VoiceBank.add: the bank is full ({self.capacity} voices)")
        i = len(self.meta)
        self._write(i, voice)
        self.meta.append(dict(clips=voice.clips, frontend=voice.frontend))
        return i

    def replace(self, i: int, voice: Voice) -> int:
        """voice `i` becomes `voice`, written at the same addresses"""
        _check_voice(voice, self.eng, "VoiceBank.replace")
        i = int(i)
        if not 0 <= i < len(self.meta):
            raise ValueError(f"VoiceBank.replace: id {i} is not one of the {len(self.meta)} voices of the bank")
        self._write(i, voice)
        self.meta[i] = dict(clips=voice.clips, frontend=voice.frontend)
        return i

    def voice(self, i: int) -> Voice:
        """a copy of voice `i`"""
        i = int(i)
        if not 0 <= i < len(self.meta):
            raise ValueError(f"VoiceBank.voice: id {i} is not one of the {len(self.meta)} voices of the bank")
        return Voice(self.z[i].clone(), self.idx[i].clone(), self.fingerprint, **self.meta[i])

    def save(self, path: str):
        """the added voices as one safetensors file (the container of stzs/checkpoint.py): tensors "z" [n, L_s, code]
        and "idx" [n, L_s, G]; format, fingerprint, capacity and the per-voice metadata in the file's metadata"""
        from safetensors.torch import save_file
        n = len(self.meta)
        save_file({"z": self.z[:n].detach().cpu().contiguous(), "idx": self.idx[:n].detach().cpu().contiguous()}, path,
                  metadata={"format": FORMAT, "fingerprint": self.fingerprint, "capacity": str(self.capacity),
                            "voices": json.dumps(self.meta)})

    @classmethod
    def load(cls, path: str, engine, capacity: int = None) -> "VoiceBank":
        """ValueError on a foreign format and on a fingerprint that is not the engine's"""
        from safetensors import safe_open
        with safe_open(path, framework="pt") as f:
            meta = f.metadata() or {}
            if meta.get("format") != FORMAT:
                raise ValueError(f"{path}: not a {FORMAT} voice bank (format={meta.get('format')!r})")
            if meta.get("fingerprint") != engine_fingerprint(engine):
                raise ValueError(f"{path}: the bank was enrolled under another prompt encoder / codebook")
            z, idx = f.get_tensor("z"), f.get_tensor("idx")
        voices = json.loads(meta["voices"])
        if z.shape[0] != len(voices) or idx.shape[0] != len(voices):
            raise ValueError(f"{path}: {z.shape[0]} voices stored, {len(voices)} described")
        cap = max(int(meta.get("capacity", "1")), len(voices), 1) if capacity is None else int(capacity)
        bank = cls(engine, cap)
        for i, m in enumerate(voices):
            bank.add(Voice(z[i].to(engine.device), idx[i].to(engine.device), meta["fingerprint"], int(m["clips"]),
                           m["frontend"]))
        return bank


def check_sources(B: int, n_voices: int, ids, weights=None):
    """the per-row sources of a batch, checked on the host -> (src [[int]], w [[float]]) per row.  ids: B voice ids
    (one voice per row; a sequence or a host tensor), or B id sequences (blends) with B weight sequences (None: equal
    weights).  ValueError for a wrong count, an id outside [0, n_voices), more than KMAX sources, a bad weight."""
    B = int(B)
    if B < 1:
        raise ValueError(f"voice_rows: B must be >= 1, got {B}")
    if isinstance(ids, torch.Tensor):
        if ids.device.type != "cpu":
            raise ValueError("voice_rows takes host ids")
        ids = ids.tolist()
    try:
        ids = list(ids)
    except TypeError:
        raise ValueError(f"voice_rows: ids must be {B} voice ids or {B} id sequences")
    if len(ids) != B:
        raise ValueError(f"voice_rows: {len(ids)} rows of ids for a batch of {B}")
    if weights is not None:
        weights = list(weights)
        if len(weights) != B:
            raise ValueError(f"voice_rows: {len(weights)} rows of weights for a batch of {B}")
    src, w = [], []
    for b, row in enumerate(ids):
        single = not isinstance(row, (list, tuple, torch.Tensor))
        row = [row] if single else list(row)
        if not 1 <= len(row) <= KMAX:
            raise ValueError(f"voice_rows: row {b} has {len(row)} sources (1 to {KMAX})")
        for k, v in enumerate(row):
            try:
                if isinstance(v, bool):
                    raise TypeError
                row[k] = operator.index(v)
            except TypeError:
                raise ValueError(f"voice_rows: row {b}: voice ids are integers, got {v!r}")
            if not 0 <= row[k] < n_voices:
                raise ValueError(f"voice_rows: row {b}: id {row[k]} is not one of the bank's {n_voices} voices")
        wr = None if weights is None else weights[b]
        if wr is not None and not isinstance(wr, (list, tuple, torch.Tensor)):
            wr = [wr]
        src.append(row)
        w.append(normalise_weights(wr, len(row), f"voice_rows: row {b} weights"))
    return src, w


class VoiceRows:
    """the speakers of one batch of B rows (StyleTTSZS.voice_rows makes them): per row 1 .. Kmax voice ids of a bank and
    their normalised weights, in device arrays this object owns -- src int32 [B, Kmax], w fp32 [B, Kmax], cnt int32 [B].
    `gather` (every row one voice: the gather form) and `Kmax` are fixed when the object is made; set() rewrites the
    arrays in place."""

    def __init__(self, B: int, bank, ids, weights=None, device=None):
        src, w = check_sources(B, len(bank), ids, weights)
        self.B, self.bank = int(B), bank
        self.device = torch.device(device) if device is not None else bank.z.device
        self.Kmax = max(len(r) for r in src)
        self.gather = self.Kmax == 1
        self.src = torch.empty(self.B, self.Kmax, dtype=torch.int32, device=self.device)
        self.w = torch.empty(self.B, self.Kmax, dtype=torch.float32, device=self.device)
        self.cnt = torch.empty(self.B, dtype=torch.int32, device=self.device)
        self.host = {}
        self._upload(src, w)

    @classmethod
    def from_device(cls, bank, src: torch.Tensor, w: torch.Tensor, cnt: torch.Tensor, gather: bool) -> "VoiceRows":
        """rows over device arrays the caller already holds (src int32 [B, Kmax], w fp32 [B, Kmax], cnt int32 [B]) --
        nothing is read back or checked on the host: the kernel clamps what it reads.  The operator path."""
        r = object.__new__(cls)
        r.B, r.bank, r.device, r.Kmax, r.gather = int(src.shape[0]), bank, src.device, int(src.shape[1]), bool(gather)
        r.src, r.w, r.cnt, r.host = src, w, cnt, {}
        return r

    def _upload(self, src, w):
        K = self.Kmax
        # (entries past a row's count are never read by the kernel: its first source, weight 0)
        hs = torch.tensor([r + [r[0]] * (K - len(r)) for r in src], dtype=torch.int32)
        hw = torch.tensor([r + [0.0] * (K - len(r)) for r in w], dtype=torch.float32)
        hc = torch.tensor([len(r) for r in src], dtype=torch.int32)
        self.src.copy_(hs)
        self.w.copy_(hw)
        self.cnt.copy_(hc)
        self.host = dict(src=hs, w=hw, cnt=hc)

    def set(self, ids, weights=None):
        """new speakers for the same batch, into the same device arrays.  ValueError -- before anything is written --
        for what voice_rows() would refuse and for a structural change: a blended row in an object made for the gather
        form, or more sources in a row than Kmax.  (An object made for the mix form takes single-voice rows: cnt 1.)"""
        src, w = check_sources(self.B, len(self.bank), ids, weights)
        kmax = max(len(r) for r in src)
        if self.gather and kmax > 1:
            raise ValueError("VoiceRows.set: these rows were made for the gather form (one voice per row); a blend is "
                             "structural: make new rows")
        if kmax > self.Kmax:
            raise ValueError(f"VoiceRows.set: {kmax} sources in a row, the rows were made for at most {self.Kmax} "
                             "(structural: make new rows)")
        self._upload(src, w)
        return self

    def rows(self, B: int):
        """these rows for a batch of B -> self (ValueError when B is not theirs)"""
        if int(B) != self.B:
            raise ValueError(f"voices were made for {self.B} rows, the batch has {B}")
        return self


class _Stack:
    """a bank-like view of stacked voices (the scheduler's per-chunk bank): z [V, L_s, code], idx [V, L_s, G]"""

    def __init__(self, voices: Sequence[Voice] = (), z: torch.Tensor = None, idx: torch.Tensor = None):
        """voices, or the stacked tensors themselves (idx may be None where only the mix form will read the bank)"""
        self.z = torch.stack([v.z for v in voices]).contiguous() if z is None else z
        self.idx = torch.stack([v.idx for v in voices]).contiguous() if z is None else idx
        self.n = int(self.z.shape[0])

    def __len__(self):
        return self.n
