"""Variable-length batching for the synthesis hot path (length bucketing).

The kernels take uniform [B, T, C] batches (per-utterance InstanceNorm statistics, LSTM recurrences and
attention are computed per row, never across rows).  Real requests differ in token count, reference length
and -- known only after the duration head -- frame count.  BucketScheduler runs them in two phases:

  phase 1  requests grouped by (token count, reference length), chunks of <= max_batch:
           text encoder, prompt front end, style diffusion, duration head (a1-a6)  -> per-utterance durations
  phase 2  utterances regrouped by their aligned frame count T40 (the quantity every decoder buffer is sized
           by), chunks of <= max_batch: alignment, prosody (a7-a8) and the decoder (a9-a13).  Token rows of a
           phase-2 batch are zero-padded to its longest text with duration 0 for the padding tokens, which the
           alignment scan never references -- so padding changes no output value.

Every row is computed exactly as it would be alone (tests/test_gpu_scheduler.py compares against
per-request synth() calls), so bucketing is a pure scheduling decision.  Regrouping copies a few small
per-utterance tensors (text rows, duration-encoder rows, codes) with torch indexing on the device: data
movement only, no compute.

ragged_text=True (off by default) drops the token count from the phase-1 key: requests sharing a reference length
run phase 1 as ONE batch padded to its longest text, each row with its own length (the engine's text_lens: row b is
computed as alone on its first text_lens[b] tokens, DESIGN.md "Ragged text batches"), and the per-utterance rows
are cut back to their own length before phase 2.  Mixed-length traffic then takes one phase-1 pass per reference
length instead of one per (token count, reference length).

ragged_ref=True (off by default) drops the reference length from the key in the same way: the references of a chunk
are zero-padded to its longest and each row's own sample count goes down as the engine's ref_lens (row b's prompt is
computed as alone on its first ref_lens[b] samples, the padding is never read: DESIGN.md §2c).  With both flags on the
key is (forced,) alone -- phase 1 is one batch per max_batch requests on any traffic; with both off the schedule is,
call for call, the uniform one.  The padded block is as wide as the chunk's longest reference: the share of it that
is padding is work this design accepts (requests are not sorted by reference length inside a chunk).

ragged_frames=True (off by default) splits phase 2: phase 2a runs alignment and prosody (a7-a8) for chunks of <=
max_batch requests in request order, whatever their frame counts -- text padded to the chunk's longest, ONE ragged
batch per chunk at the padded width of its longest row (the engine's ragged_frames: row b is computed as alone on its
own T_b frames); phase 2b groups by T40 as before, cuts each bucket's rows out of the prosody results
(engine.prosody_rows: data movement only) and runs the decoder per bucket.  With it off the schedule is, call for
call, the present one.

ragged_decoder=True (off by default; requires ragged_frames) keeps phase 2 in one piece again, now on ragged batches:
the requests are sorted by their frame count (known on the host after phase 1; neighbours in the order share the least
padding) and cut into chunks of <= max_batch; each chunk runs ONE ragged prosody batch and ONE ragged decoder pass on
its result (the engine's decode(frame_lens=...): row b is computed as alone on its own T_b frames) --
no per-row copies -- and request i's waveform is the first 600 T40_i samples of its row.

Per-request controls: a Request carries its own guidance scale (None: the scheduler's), speaking rate and
pitch shift.  They are no part of any grouping key: a phase-1 chunk with a request off the defaults runs with ONE
RowControls (guidance, rate -- the engine's row_controls), a phase-2 chunk with a shifted request with one for the
pitch; every row is still computed as alone with its own values.  A chunk of all-default requests makes, call for
call, the calls from before the controls existed (stats["control_batches"] counts the batches that took controls).

Sample rates: a Request may carry the rate of its reference (ref_sr) and the rate it wants its
waveform at (out_sr).  Before phase 1 the references of each distinct foreign ref_sr are padded to the longest of them
and converted in ONE ragged launch (the engine's resample(lens=...): row b the bits of its own conversion); each
request goes on with its own-length reference at the model's rate, so the grouping keys see those lengths.  After phase
2 the waveforms of each distinct foreign out_sr are converted the same way.  stats["resample_batches"] counts both; a
list of requests at the defaults makes, call for call, the calls from before.

Enrolled voices: a Request may name its speaker as a Voice (engine.enroll), or as a blend -- a sequence
of (Voice, weight) pairs -- in place of ref_wav.  Such requests have no reference length: their phase-1 key holds a
constant in its place, whatever the flags, so they batch together and never with waveform requests.  Per chunk the
distinct Voice objects (by identity, in first-appearance order) are stacked into one bank, ONE VoiceRows is made and the
prompt is ONE stzs_voice_prompt launch: data movement only, as the regrouping.  stats["voice_batches"] counts those
chunks; a list without voices makes, call for call, the calls from before.
"""
from __future__ import annotations

import dataclasses
import time
from functools import partial
from collections import OrderedDict
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import resample as RS
from . import voice as VC
from .engine import Act, StyleTTSZS


@dataclass
class Request:
    tokens: torch.Tensor            # int [T_txt]
    ref_wav: Optional[torch.Tensor]  # fp32 [N] reference (at 24 kHz, or at ref_sr); None with `voice`
    noise: torch.Tensor             # fp32 [L_s, code_dim] style noise
    seed: int = 0                   # harmonic-source noise seed
    durations: Optional[torch.Tensor] = None  # optional forced int [T_txt]
    cfg_scale: Optional[float] = None  # guidance scale (None: the scheduler's)
    speed: float = 1.0              # speaking rate: predicted durations are divided by it
    pitch_shift: float = 0.0        # semitones: F0 is multiplied by 2 ** (pitch_shift / 12)
    ref_sr: Optional[int] = None    # the rate of ref_wav (None: the model's 24 kHz)
    out_sr: Optional[int] = None    # the rate of the returned waveform (None: the model's)
    voice: object = None            # an enrolled Voice, or a sequence of (Voice, weight) pairs (a blend): no ref_wav


def request_voices(r):
    """the (Voice, weight) pairs of a request's `voice` field -> ([Voice], [weight] | None); None for a waveform
    request.  ValueError for a request with both a voice and a reference (or a ref_sr), with neither, for a blend that
    is empty or holds something else than (Voice, weight) pairs."""
    v = getattr(r, "voice", None)
    if v is None:
        if r.ref_wav is None:
            raise ValueError("Request: neither ref_wav nor voice is given")
        return None
    if r.ref_wav is not None or getattr(r, "ref_sr", None) is not None:
        raise ValueError("Request: voice and ref_wav / ref_sr were both given: the speaker comes from one or the other")
    if isinstance(v, VC.Voice):
        return [v], None
    try:
        pairs = [(a, float(b)) for a, b in v]
    except (TypeError, ValueError):
        raise ValueError("Request.voice must be a Voice or a sequence of (Voice, weight) pairs")
    if not pairs or any(not isinstance(a, VC.Voice) for a, _ in pairs):
        raise ValueError("Request.voice must be a Voice or a sequence of (Voice, weight) pairs")
    return [a for a, _ in pairs], [b for _, b in pairs]


class Stats(dict):
    """BucketScheduler.stats.  A counter that came with a per-request option and is zero for a list of requests that
    does not use the option is not listed -- the statistics of such a list are, key for key, the ones from before the
    option -- and reads as 0."""
    OPTIONAL = ("resample_batches", "voice_batches")

    def __missing__(self, key):
        if key in self.OPTIONAL:
            return 0
        raise KeyError(key)


class BucketScheduler:
    def __init__(self, engine: StyleTTSZS, max_batch: int = 64, steps: int = 2, cfg_scale: float = 5.0,
                 ragged_text: bool = False, ragged_ref: bool = False, ragged_frames: bool = False,
                 ragged_decoder: bool = False):
        if ragged_decoder and not ragged_frames:
            raise ValueError("ragged_decoder requires ragged_frames (the ragged decoder reads the ragged prosody's rows)")
        if ragged_frames:
            engine._check_ragged_frames()  # (NotImplementedError on the latency / precise engines, before any launch)
        if ragged_decoder:
            engine._check_ragged_decoder()  # (... and on a spec whose generator convs do not take the lengths)
        self.eng, self.max_batch, self.steps, self.cfg = engine, max_batch, steps, cfg_scale
        self.ragged_text, self.ragged_ref, self.ragged_frames = ragged_text, ragged_ref, bool(ragged_frames)
        self.ragged_decoder = bool(ragged_decoder)
        self.stats = {}

    def _chunks(self, ids):
        for i in range(0, len(ids), self.max_batch):
            yield ids[i:i + self.max_batch]

    def phase1_groups(self, reqs: List[Request]):
        """the phase-1 batches of reqs, in launch order -> [(forced durations?, [request indices])], each of at most
        max_batch requests that share (token count, reference length, forced); ragged_text takes the token count out
        of the key, ragged_ref the reference length (both: (forced,) alone).  A request that names an enrolled voice has
        the constant "voice" where the reference length stands, whatever ragged_ref says: voice requests share batches
        among themselves and never with waveform requests.  Pure host bookkeeping (reads shapes only)."""
        g1 = OrderedDict()
        for i, r in enumerate(reqs):
            key = (r.durations is not None,)
            if request_voices(r) is not None:
                key = ("voice",) + key
            elif not self.ragged_ref:
                key = (int(r.ref_wav.shape[0]),) + key
            if not self.ragged_text:
                key = (int(r.tokens.shape[0]),) + key
            g1.setdefault(key, []).append(i)
        return [(key[-1], ch) for key, ids in g1.items() for ch in self._chunks(ids)]

    def phase2_groups(self, frames: List[int]):
        """the phase-2 batches for the requests' frame counts, in launch order -> (prosody batches, decoder batches),
        each a list of request-index lists of at most max_batch.  Without ragged_frames a batch shares its T40 and
        runs prosody and decoder together (the two lists are the same); with it the prosody batches are chunks of the
        requests in request order and only the decoder batches share a T40; with ragged_decoder as well, both lists
        are the chunks of the requests sorted by T40 (a stable sort).  Pure host bookkeeping."""
        if self.ragged_decoder:
            ch = list(self._chunks(sorted(range(len(frames)), key=lambda i: int(frames[i]))))
            return ch, ch
        g2 = OrderedDict()
        for i, n in enumerate(frames):
            g2.setdefault(int(n), []).append(i)
        dec = [ch for ids in g2.values() for ch in self._chunks(ids)]
        if not self.ragged_frames:
            return dec, dec
        return list(self._chunks(list(range(len(frames))))), dec

    def _resample_groups(self, items, sr_of, to_model: bool):
        """one ragged conversion per distinct foreign rate: items {index: fp32 [n] tensor}, sr_of(index) its other
        rate -> {index: converted own-length tensor} for the indices at a foreign rate (the others are left out)"""
        eng, S, dev = self.eng, self.eng.spec, self.eng.device
        groups = OrderedDict()
        for i in items:
            sr = sr_of(i)
            if sr is not None and int(sr) != S.sr:
                groups.setdefault(int(sr), []).append(i)
        done = {}
        for sr, ids in groups.items():
            nl = [int(items[i].shape[0]) for i in ids]
            Nm = max(nl)
            x = torch.stack([torch.nn.functional.pad(items[i].to(dev, torch.float32), (0, Nm - items[i].shape[0]))
                             for i in ids])
            a, b = (sr, S.sr) if to_model else (S.sr, sr)
            y, _ = eng.resample(x, a, b, lens=nl if min(nl) < Nm else None)
            self._nrs += 1
            for j, i in enumerate(ids):
                done[i] = y[j, :RS.out_len(nl[j], *RS.ratio(a, b))].clone()
        return done

    def _voice_rows(self, items):
        """the speakers of one phase-1 chunk: items [([Voice], [weight] | None)] per request -> VoiceRows over a bank
        stacked from the chunk's distinct Voice objects (by identity, in first-appearance order).  Data movement only."""
        order, pos = [], {}
        for vs, _ in items:
            for v in vs:
                if id(v) not in pos:
                    VC._check_voice(v, self.eng, "Request.voice")
                    pos[id(v)] = len(order)
                    order.append(v)
        ids = [[pos[id(v)] for v in vs] for vs, _ in items]
        if all(len(r) == 1 for r in ids):
            return self.eng.voice_rows(len(items), VC._Stack(order), [r[0] for r in ids])
        return self.eng.voice_rows(len(items), VC._Stack(order), ids, [ws for _, ws in items])

    def _phase1_controls(self, reqs, ch):
        """the guidance / rate controls of phase-1 chunk ch -> RowControls, or None when every request of it is at the
        defaults (the scheduler's guidance scale, rate 1).  A guidance scale the whole chunk shares goes down as a
        scalar (the engine's scalar path), different ones as one value per row."""
        cfg = [self.cfg if reqs[i].cfg_scale is None else float(reqs[i].cfg_scale) for i in ch]
        speed = [float(getattr(reqs[i], "speed", 1.0)) for i in ch]
        mixed = any(c != cfg[0] for c in cfg)
        rated = any(r != 1.0 for r in speed)
        if not mixed and not rated and cfg[0] == self.cfg:
            return None
        return self.eng.row_controls(len(ch), cfg_scale=cfg if mixed else cfg[0], speed=speed if rated else None)

    def _phase2_controls(self, per, ch):
        """the pitch controls of phase-2 chunk ch -> dict(controls=RowControls), or {} when no request of it is
        shifted (the call then is the one from before the controls)"""
        pitch = [per[i]["pitch"] for i in ch]
        if all(p == 0.0 for p in pitch):
            return {}
        self._nctl += 1
        return dict(controls=self.eng.row_controls(len(ch), pitch_shift=pitch))

    def _phase2_inputs(self, per, ch):
        """the padded text rows / duration-encoder rows / durations and the codes of requests ch"""
        dev = self.eng.device
        Tm = max(per[i]["h"].shape[0] for i in ch)
        b = len(ch)
        h = torch.zeros(b, Tm, per[ch[0]]["h"].shape[1], dtype=per[ch[0]]["h"].dtype, device=dev)
        d = torch.zeros(b, Tm, per[ch[0]]["d"].shape[1], dtype=per[ch[0]]["d"].dtype, device=dev)
        dur = torch.zeros(b, Tm, dtype=torch.int32, device=dev)
        for j, i in enumerate(ch):
            T = per[i]["h"].shape[0]
            h[j, :T], d[j, :T], dur[j, :T] = per[i]["h"], per[i]["d"], per[i]["dur"]
        codes = torch.stack([per[i]["codes"] for i in ch]).contiguous()
        return h, d, dur, codes

    def _phase2_ragged(self, per, out):
        """phase 2a (one ragged prosody batch per chunk of requests) and 2b (decoder per frame bucket)
        -> (prosody batches, decoder batches, padded frame blocks, of them tail)"""
        eng, S = self.eng, self.eng.spec
        pros, dec = self.phase2_groups([p["T40"] for p in per])
        fr_n = pad_n = 0
        for ch in pros:
            h, d, dur, codes = self._phase2_inputs(per, ch)
            Tp = max(per[i]["T40"] for i in ch)
            pro = eng.prosody_frames(Act(h, 0, S.d_txt), codes, Act(d, 0, S.pr_in), dur, Tp, ragged_frames=True,
                                     **self._phase2_controls(per, ch))
            fr_n += Tp * len(ch)
            pad_n += Tp * len(ch) - sum(per[i]["T40"] for i in ch)
            # each row's prosody cut out before the next chunk reuses the buffers (data movement only)
            for j, i in enumerate(ch):
                per[i]["pro"] = eng.prosody_rows(pro, [j], per[i]["T40"])
        for ch in dec:
            T40 = per[ch[0]]["T40"]
            asr = torch.cat([per[i]["pro"]["asr_buf"].t for i in ch])
            pro = dict(asr_buf=Act(asr, 0, S.d_txt + 2), F0=torch.cat([per[i]["pro"]["F0"] for i in ch]),
                       N=torch.cat([per[i]["pro"]["N"] for i in ch]), T40=T40)
            codes = torch.stack([per[i]["codes"] for i in ch]).contiguous()
            wav = eng.decode(pro, codes, [per[i]["seed"] for i in ch])
            for j, i in enumerate(ch):
                out[i] = wav[j].clone()
        return len(pros), len(dec), fr_n, pad_n

    def _phase2_ragged_decoder(self, per, out):
        """phase 2 with the ragged decoder: per chunk of requests (sorted by frame count) one ragged prosody batch and
        one ragged decoder pass on it -> (batches, padded frame blocks, of them tail)"""
        eng, S = self.eng, self.eng.spec
        chunks, _ = self.phase2_groups([p["T40"] for p in per])
        fr_n = pad_n = 0
        for ch in chunks:
            h, d, dur, codes = self._phase2_inputs(per, ch)
            Tp = max(per[i]["T40"] for i in ch)
            pro = eng.prosody_frames(Act(h, 0, S.d_txt), codes, Act(d, 0, S.pr_in), dur, Tp, ragged_frames=True,
                                     **self._phase2_controls(per, ch))
            wav = eng.decode(pro, codes, [per[i]["seed"] for i in ch], frame_lens=pro["frame_lens"])
            fr_n += Tp * len(ch)
            pad_n += Tp * len(ch) - sum(per[i]["T40"] for i in ch)
            n = S.frame40  # samples per 40-fps frame
            for j, i in enumerate(ch):
                out[i] = wav[j, :n * per[i]["T40"]].clone()
        return len(chunks), fr_n, pad_n

    def synth(self, reqs: List[Request]) -> List[torch.Tensor]:
        """-> one fp32 waveform [600 * T40_i] per request (at its out_sr: [ceil(600 T40_i out_sr / sr)]), in request
        order (device tensors)."""
        eng, S, dev = self.eng, self.eng.spec, self.eng.device
        self._nrs = 0  # ragged sample-rate conversions
        out_srs = [getattr(r, "out_sr", None) for r in reqs]
        voiced = [request_voices(r) for r in reqs]  # (checks every request before anything is launched)
        refs = self._resample_groups({i: r.ref_wav for i, r in enumerate(reqs) if voiced[i] is None},
                                     lambda i: getattr(reqs[i], "ref_sr", None), True)
        if refs:  # the requests go on with their references at the model's rate (the caller's are left as they are);
            # the converted ones live on the device, so the others of the list are taken there too: one batch stacks both
            reqs = [r if voiced[i] is not None else
                    dataclasses.replace(r, ref_wav=refs[i] if i in refs else r.ref_wav.to(dev), ref_sr=None)
                    for i, r in enumerate(reqs)]
        # ---- phase 1: text / prompt / style / durations, grouped by (T_txt, N_ref) -- ragged_text: without T_txt,
        # ragged_ref: without N_ref ----
        per = [None] * len(reqs)
        n1 = 0
        self._nctl = 0  # batches that ran with controls
        nvoice = 0  # phase-1 batches whose prompt came from enrolled voices
        ref_n = pad_n = 0  # reference samples of the phase-1 blocks, and how many of them are padding
        t1 = time.perf_counter()  # (every phase-1 batch ends in a host sync: the wall time is the phase's)
        for forced, ch in self.phase1_groups(reqs):
            n1 += 1
            tl = [int(reqs[i].tokens.shape[0]) for i in ch]
            Tm = max(tl)
            lens = None
            if self.ragged_text and min(tl) < Tm:
                # pad to the chunk's longest text (any valid symbol: the padding is never read; durations 0) and
                # hand the rows' own lengths to the engine: checked on the host and uploaded once
                pad = lambda v: torch.nn.functional.pad(v, (0, Tm - v.shape[0]))
                tok = torch.stack([pad(reqs[i].tokens) for i in ch]).to(dev, torch.int32)
                dur_ov = torch.stack([pad(reqs[i].durations) for i in ch]) if forced else None
                lens = eng.text_lens(tl, len(ch), Tm)
            else:
                tok = torch.stack([reqs[i].tokens for i in ch]).to(dev, torch.int32)
                dur_ov = torch.stack([reqs[i].durations for i in ch]) if forced else None
            vr = ref = rlens = None
            # (a chunk is all voices or all waveforms: the key keeps them apart; voices have no reference samples)
            nl = [0] if voiced[ch[0]] is not None else [int(reqs[i].ref_wav.shape[0]) for i in ch]
            Nm = max(nl)
            if voiced[ch[0]] is not None:
                vr = self._voice_rows([voiced[i] for i in ch])
                nvoice += 1
            elif self.ragged_ref and min(nl) < Nm:
                # pad to the chunk's longest reference (zeros: never read) and hand the rows' own sample counts down
                ref = torch.stack([torch.nn.functional.pad(reqs[i].ref_wav, (0, Nm - reqs[i].ref_wav.shape[0]))
                                   for i in ch]).to(dev, torch.float32)
                rlens = eng.ref_lens(nl, len(ch), Nm)
                pad_n += Nm * len(ch) - sum(nl)
            else:
                ref = torch.stack([reqs[i].ref_wav for i in ch]).to(dev, torch.float32)
            ref_n += Nm * len(ch)
            eps = torch.stack([reqs[i].noise for i in ch]).to(dev, torch.float32)
            # the prompt of the chunk: the front end on its references, or one launch on its enrolled voices
            prompt_of = (lambda **kw: eng.voice_encode(vr)) if vr is not None else partial(eng.prompt_encode, ref)
            rc = self._phase1_controls(reqs, ch)
            if rc is not None:
                self._nctl += 1
                h = eng.text_encode(tok, lens)
                prompt = prompt_of(ref_lens=rlens)
                codes = eng.sample_style(h, prompt, eps, self.steps, self.cfg, lens, controls=rc)
                du = eng.predict_durations(h, codes, dur_ov, lens, controls=rc)
            elif lens is None and rlens is None:  # (the uniform path, call for call as before)
                h = eng.text_encode(tok)
                prompt = prompt_of()
                codes = eng.sample_style(h, prompt, eps, self.steps, self.cfg)
                du = eng.predict_durations(h, codes, dur_ov)
            else:
                h = eng.text_encode(tok, lens)
                prompt = prompt_of(ref_lens=rlens)
                codes = eng.sample_style(h, prompt, eps, self.steps, self.cfg, lens)
                du = eng.predict_durations(h, codes, dur_ov, lens)
            tot = du["dur"].to(torch.int64).sum(1).cpu()  # host sync: frame counts decide phase 2
            eng.check_status()  # a timed-out LSTM exchange would make these durations wrong: raise
            for j, i in enumerate(ch):
                T = tl[j]  # the row's own text: what lies past it in a ragged batch is padding
                per[i] = dict(h=h.t[j, :T].clone(), d=du["d"].t[j, :T].clone(), dur=du["dur"][j, :T].clone(),
                              codes=codes[j].clone(), T40=int(tot[j]), seed=reqs[i].seed,
                              pitch=float(getattr(reqs[i], "pitch_shift", 0.0)))
        t1 = time.perf_counter() - t1
        # ---- phase 2: prosody + decoder, grouped by aligned frame count ----
        g2 = OrderedDict()
        for i, p in enumerate(per):
            g2.setdefault(p["T40"], []).append(i)
        out = [None] * len(reqs)
        n2 = 0
        npro, fr_n, fpad_n = None, 0, 0
        if self.ragged_decoder:
            n2, fr_n, fpad_n = self._phase2_ragged_decoder(per, out)
            npro = n2
        elif self.ragged_frames:
            npro, n2, fr_n, fpad_n = self._phase2_ragged(per, out)
        for T40, ids in ([] if self.ragged_frames else g2.items()):
            for ch in self._chunks(ids):
                n2 += 1
                Tm = max(per[i]["h"].shape[0] for i in ch)
                b = len(ch)
                h = torch.zeros(b, Tm, per[ch[0]]["h"].shape[1], dtype=per[ch[0]]["h"].dtype, device=dev)
                d = torch.zeros(b, Tm, per[ch[0]]["d"].shape[1], dtype=per[ch[0]]["d"].dtype, device=dev)
                dur = torch.zeros(b, Tm, dtype=torch.int32, device=dev)
                for j, i in enumerate(ch):
                    T = per[i]["h"].shape[0]
                    h[j, :T], d[j, :T], dur[j, :T] = per[i]["h"], per[i]["d"], per[i]["dur"]
                codes = torch.stack([per[i]["codes"] for i in ch]).contiguous()
                pro = eng.prosody_frames(Act(h, 0, S.d_txt), codes, Act(d, 0, S.pr_in), dur, T40,
                                         **self._phase2_controls(per, ch))
                wav = eng.decode(pro, codes, [per[i]["seed"] for i in ch])
                for j, i in enumerate(ch):
                    out[i] = wav[j].clone()
        eng.check_status()  # the phase-2 prosody LSTMs
        for i, w in self._resample_groups({i: w for i, w in enumerate(out)}, lambda i: out_srs[i], False).items():
            out[i] = w
        self.stats = Stats(requests=len(reqs), phase1_batches=n1, phase2_batches=n2, control_batches=self._nctl,
                          frame_buckets=sorted(g2.keys()), phase1_ms=1e3 * t1,
                          ref_pad_share=pad_n / max(ref_n, 1),
                          # prosody batches (ragged_frames: fewer than the decoder's; else one per phase-2 batch) and
                          # the share of the padded prosody frame blocks that is tail
                          prosody_batches=n2 if npro is None else npro, frame_pad_share=fpad_n / max(fr_n, 1),
                          # decoder passes, and the share of their padded frame blocks that is tail (ragged_decoder:
                          # the prosody's; else a decoder batch shares its frame count)
                          decoder_batches=n2, decoder_pad_share=fpad_n / max(fr_n, 1) if self.ragged_decoder else 0.0)
        if self._nrs:  # (the ragged sample-rate conversions, both directions; reads as 0 where it is not listed)
            self.stats["resample_batches"] = self._nrs
        if nvoice:  # (likewise)
            self.stats["voice_batches"] = nvoice
        return out
