"""StyleTTS-ZS synthesis engine on MI355X: the L4 host pipeline over libstzs_hip.so.

API (the upstream inference API is "Under construction",
`/root/reference/README.md:15-16`, so this pins it in the StyleTTS2-family shape
`inference(text, ref_s, diffusion_steps, embedding_scale)`):

    eng = StyleTTSZS(spec, params, device="cuda:0")
    out = eng.synth(tokens, ref_wav, steps=2, cfg_scale=5.0, noise=eps, durations=dur)
    codes = eng.sample_style(h_txt, prompt, eps, steps, cfg_scale)     # (a) style diffusion
    pro   = eng.predict_prosody(h_txt, codes, durations)               # (b) duration/prosody
    wav   = eng.decode(pro, codes, seeds)                              # (c) iSTFT decoder

Every FLOP of synth() -- including the reference-prompt front end (log-mel + prompt encoder, SURVEY
§8(f) rank 1) -- runs in a hand-written gfx950 kernel reached through the C-ABI; PyTorch only
provides device memory (caching allocator) and the stream.  Buffers are cached per shape so a whole
synth() can be captured into one HIP graph (`capture()`), which removes all host launch overhead.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from functools import partial

import numpy as np
import torch

from . import _lib as L
from . import resample as RS
from . import voice as VC
from .spec import Spec
from .weights import ConvW, PackedModel

_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float8_e4m3fn: L.F8}
# split-K slices per bf16 denoiser layer linear (stzs_conv_args.splitk), a per-engine setting.  At batch 1 (100
# rows with CFG) ffn2 has 8 output tiles, each streaming its 64 K-steps through one CU's LDS-DMA ring; 4 slices
# spread that over 32 CUs (14.9 -> 10.5 us; configs[1] p50 10.1 -> 9.9 ms).  The K = 512 linears lose (the hand-off
# costs more than their 16 K-steps), and so does every linear at 6 400 rows (ffn2 26.7 -> 40.5 us; bench value
# -1.5%), so throughput engines keep it off (DN_SPLITK) and the batch-1 latency engine uses LATENCY_DN_SPLITK
# (tools/gemm_bench.py, DESIGN.md §5 "Batch-1 latency").  Within one engine the table is a property of the weight,
# applied at every row count, so its results stay batch-invariant.  STZS_DN_SPLITK overrides the default of an
# engine built without dn_splitk: "0" = off, or e.g. "ff2=4,o=2".
DN_SPLITK = {}
LATENCY_DN_SPLITK = dict(ff2=4)
# small-M linears on the whole chip (csrc/rows.hip, STZS_CONV_ROWS): per denoiser linear the number of K slices Z
# (1 = no split).  The batch-1 latency engine's table; like the split-K table it is a property of the weight applied
# at every row count (batch-invariant), and it takes precedence over dn_splitk.  STZS_DN_ROWS overrides the default
# ({}): "0" = off, or e.g. "qkv=1,ff2=4".
DN_ROWS = {}
LATENCY_DN_ROWS = dict(inp=1, qkv=1, o=1, q=1, co=1, ff1=1, ff2=4, out=1)
# in-launch split-K (input-channel chunks, csrc/conv.hip conv_mfma) of the text-encoder k5 convs: at batch 1 their
# grid is 4 workgroups of 80 K-steps each.  A per-engine property of the weight (batch-invariant); the batch-1
# latency engine's value.  STZS_TE_SPLITK overrides an engine built without te_splitk.
TE_SPLITK = 0
LATENCY_TE_SPLITK = 4
# split-K slices of the decoder / predictor AdaIN-block convs (their generic-layout copies, BlkW.conv1s / conv2s) in
# the batch-1 latency engine: at 200-400 frames a decoder conv is 16 tiles x 108 K-steps on 16 CUs; 0 = off.  16 (r05)
# = one input-channel chunk per slice for every block conv (<= 9 chunks): the DEEP form (csrc/conv.hip)
BLK_SPLITK = 0
LATENCY_BLK_SPLITK = 16


_ES = {L.F32: 4, L.BF16: 2, L.F8: 1}


def _ln_cost(a):
    """(FLOP, bytes) of a row LayerNorm launch: the rows read once and written once (the FLOPs are negligible)."""
    return 0, a.R * a.C * (_ES[a.in_dtype] + _ES[a.out_dtype])


def _conv_cost(cw, x: "Act", y: "Act", T_out, res, acc_in, ln=None):
    """(FLOP, bytes) of a conv launch; ln: the LayerNorm (stzs_rowln_args) fused in front of it."""
    flops = 2.0 * y.B * T_out * (cw.ups or 1) * cw.Co * cw.Ci * cw.ks
    if cw.wx3 is not None:  # precise mode: 3 bf16 MFMA products per fp32 product (bf16x3-equivalent FLOP)
        flops *= 3.0
    # algorithmic bytes: input tile once + output once (+ residual/acc reads), bf16/f32 as stored, + the
    # weights once (bf16; e4m3 for the fp8 linears; hi + lo for the split-operand precise form)
    wbytes = (cw.ups or 1) * cw.Co * cw.Ci * cw.ks * (1 if cw.f8 else (4 if cw.wx3 is not None else 2))
    opnd = lambda v: v.B * v.T * v.C * v.t.element_size() if v is not None else 0
    byt = opnd(x) + y.B * T_out * (cw.ups or 1) * cw.Co * y.t.element_size() + opnd(res) + opnd(acc_in) + wbytes
    if ln is not None:  # the LayerNorm's input rows instead of x
        byt += ln.R * ln.C * (4 if ln.in_dtype == L.F32 else 2) - opnd(x)
    return flops, byt


# conv flag bits that take a conv off the generic path (csrc/conv.hip conv_mfma): the LDS-DMA GEMM (8 =
# STZS_CONV_A_DMA), the small-M rows form and every weight form with a kernel of its own
_CONV_NOT_GENERIC = (8 | L.CONV_ROWS | L.CONV_W_X3 | L.CONV_W_F32 | L.CONV_W_FRAG32 | L.CONV_W_LANE16 |
                     L.CONV_W_NARROW32 | L.CONV_W_FRAG32X3)


def _conv_generic(flags, cw) -> bool:
    """the conv with these flags runs on the generic path (which splits K over input-channel chunks and finalises
    deferred prologue statistics itself)"""
    return not (flags & _CONV_NOT_GENERIC) and not cw.f8


def _table(v):
    """a per-linear table knob: a dict, or its environment form -- "0" = off, or e.g. "ff2=4,o=2" """
    if not isinstance(v, str):
        return dict(v)
    if v.strip() in ("", "0"):
        return {}
    return {k: int(n) for k, n in (kv.split("=") for kv in v.split(","))}


def _on(v):
    return v != "0"


# the per-engine knobs: (attribute, environment variable, default, parser).  A constructor argument of the attribute's
# name takes precedence over the environment; a callable default is evaluated on the engine (after the rows above it).
_KNOBS = (
    ("dur_overlap", "STZS_DUR_OVERLAP", "1", lambda v: bool(int(v))),
    # split-K of the bf16 denoiser layer linears (stzs_conv_args.splitk): a property of the weight, used at
    # every batch size so results stay batch-invariant; {} turns it off
    ("dn_splitk", "STZS_DN_SPLITK", DN_SPLITK, _table),
    # small-M whole-chip form of the bf16 denoiser linears (csrc/rows.hip): {linear: K slices}; a per-engine
    # property of the weight like dn_splitk (batch-invariant), taking precedence over it
    ("dn_rows", "STZS_DN_ROWS", DN_ROWS, _table),
    # split-K slices of the text-encoder convs (LATENCY_TE_SPLITK); 0 = off
    ("te_splitk", "STZS_TE_SPLITK", TE_SPLITK, int),
    # split-K slices of the bf16 AdaIN-block convs (LATENCY_BLK_SPLITK); 0 = the register-direct form
    ("blk_splitk", "STZS_BLK_SPLITK", BLK_SPLITK, int),
    # InstanceNorm statistics of <= 8 partial chunks handed to the consuming generic-path conv unfinalised
    # (stzs_conv_args.pro_part: the prologue finalises them, bit-identical, one launch less per statistics) --
    # the engines whose AdaIN-block convs run the generic path (blk_splitk); STZS_DEFER_STATS=0|1 overrides
    ("defer_stats", "STZS_DEFER_STATS", lambda eng: "1" if eng.blk_splitk else "0", _on),
    # (r06) small batches (<= 4 utterances): the generator MRF's three resblocks advanced side by side, each layer's
    # three convs in one launch (stzs_conv1d_group, csrc/mrfv.hip mrfv_trio) -- bit-identical; STZS_MRF_TRIO=0: off
    ("mrf_trio", "STZS_MRF_TRIO", "1", _on),
    # (r06) the batch-1 engine (blk_splitk): the prosody predictor's F0 and N branches in lockstep, each conv pair
    # in one launch pair (stzs_conv1d_group -> conv_mfma_pair) -- bit-identical; STZS_F0N_PAIR=0: off
    ("f0n_pair", "STZS_F0N_PAIR", "1", _on),
    # (r06) the denoiser layers' cross-attention K / V projections as one stacked linear; STZS_KV_FUSE=0: per layer
    ("kv_fuse", "STZS_KV_FUSE", "1", _on),
    # the per-utterance linears (one row per utterance or per sigma step: the sigma-embedding MLP, the pooled-
    # prompt projection, the decoder / predictor AdaIN gamma-beta GEMMs) on the whole-chip small-M form at every
    # batch size (a per-weight choice: batch-invariant); on the tiled GEMM they ran on 1-4 workgroups each.
    # STZS_SMALL_ROWS=0 turns it off.
    ("small_rows", "STZS_SMALL_ROWS", "1", _on),
    # with the denoiser linears on the small-M rows form (dn_rows): each adaLN / affine LayerNorm fused into the
    # one linear that reads it (stzs_ln_linear, csrc/lnrows.hip) instead of its own launch.  STZS_LN_FUSE=0: off
    ("ln_fuse", "STZS_LN_FUSE", "1", _on),
    # rows-form linears with K <= rows16_maxk on the 16-row register-direct form (csrc/lnrows.hip rows16: up to 16
    # K-steps of both operands in flight, no cross-wave reduction, no K slices).  STZS_ROWS16=0: csrc/rows.hip
    ("rows16", "STZS_ROWS16", "1", _on),
    ("rows16_split", "STZS_ROWS16_SPLIT", "1", _on),  # (the Z-slice form: batch-1 ffn2)
    # (unsliced up to K 512: ffn2, K 2048, as one 64-K-step chain measured no faster than rows.hip Z 4, r04_t;
    # with its 4 slices on the split form it is, r04_x)
    ("rows16_maxk", "STZS_ROWS16_MAXK", "512", int),
    # the last generator stage's noise conv fused into its ConvTranspose (bf16 engines); STZS_UPS_NOISE=0: off
    ("ups_noise_fused", "STZS_UPS_NOISE", "1", _on),
    # the first stage's strided noise conv on super-rows of the harmonic source (register-direct kernel, bf16
    # engines); STZS_NOISE_SUPER=0: the stride-6 conv_mfma form
    ("noise_super", "STZS_NOISE_SUPER", "1", _on),
    # precise mode: the FRAG32 convs (MRF, AdaIN-block k3) on the split-operand register-direct kernel
    # (csrc/mrfx.hip) instead of the LDS-ring conv_x3; STZS_MRFX=0: conv_x3
    ("mrfx", "STZS_MRFX", "1", _on),
    # diagnostic conv flag bits ORed into every stzs_conv1d call (e.g. STZS_CONV_LINEAR_IDS = 128)
    ("conv_flags", "STZS_CONV_FLAGS", "0", lambda v: int(v, 0)),
)


def _rup(x, m):
    return (x + m - 1) // m * m


@dataclass
class Act:
    """channels-last activation view: buffer [B, T, ld], logical channels [c0, c0 + C)."""
    t: torch.Tensor
    c0: int = 0
    C: int = -1

    def __post_init__(self):
        if self.C < 0:
            self.C = self.t.shape[-1] - self.c0

    @property
    def B(self):
        return self.t.shape[0]

    @property
    def T(self):
        return self.t.shape[1]

    @property
    def ld(self):
        return self.t.shape[2]

    @property
    def bs(self):
        """batch stride in elements: the tensor's own (a view of the first T rows of a longer buffer -- the harmonic
        source's -- keeps the buffer's stride; for contiguous buffers this is T * ld)"""
        return self.t.stride(0)

    @property
    def ptr(self):
        return self.t.data_ptr() + self.c0 * self.t.element_size()

    @property
    def dt(self):
        return _DT[self.t.dtype]

    def sl(self, c0, C):
        return Act(self.t, self.c0 + c0, C)

    def rows(self, b0, nb):
        return Act(self.t[b0:b0 + nb], self.c0, self.C)


def check_text_lens(text_lens, B: int, T: int) -> torch.Tensor:
    """host-side check of a ragged batch's per-row text lengths -> int32 [B] host tensor.  text_lens: a host
    tensor or a sequence of B integers, each in [1, T] (T the padded width); anything else raises ValueError.
    (A device tensor is never checked -- that would be a sync -- the kernels clamp what they read.)"""
    t = torch.as_tensor(text_lens)
    if t.device.type != "cpu":
        raise ValueError("check_text_lens takes host lengths")
    if t.dim() != 1 or t.shape[0] != B or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"text_lens must be {B} integers (one per row), got {tuple(t.shape)} {t.dtype}")
    if B and (int(t.min()) < 1 or int(t.max()) > T):
        raise ValueError(f"text_lens must lie in [1, {T}] (the padded width), got {t.tolist()}")
    return t.to(torch.int32)


def check_ref_lens(ref_lens, B: int, N: int, n_fft: int) -> torch.Tensor:
    """host-side check of a ragged reference batch's per-row sample counts -> int32 [B] host tensor.  ref_lens: a
    host tensor or a sequence of B integers, each in [n_fft / 2 + 1, N] (the shortest clip the STFT's reflect padding
    is defined on; N the padded width of ref_wav); anything else raises ValueError.  (A device tensor is never
    checked -- that would be a sync -- the kernels clamp what they read.)"""
    t = torch.as_tensor(ref_lens)
    if t.device.type != "cpu":
        raise ValueError("check_ref_lens takes host lengths")
    if t.dim() != 1 or t.shape[0] != B or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"ref_lens must be {B} integers (one per reference row), got {tuple(t.shape)} {t.dtype}")
    lo = n_fft // 2 + 1
    if B and (int(t.min()) < lo or int(t.max()) > N):
        raise ValueError(f"ref_lens must lie in [{lo}, {N}] (reflect padding needs more than n_fft / 2 samples; "
                         f"{N} is the padded width), got {t.tolist()}")
    return t.to(torch.int32)


def check_frame_lens(frame_lens, B: int, T40: int) -> list:
    """the ragged chunked decoder's per-row frame counts as host integers -> list of B ints.  frame_lens: a sequence or
    a host tensor of B integers, each in [1, T40] (T40 the padded width), anything else raises ValueError; or a device
    tensor, read back here -- ONE host sync, the window schedule is made on the host -- and checked the same way."""
    t = torch.as_tensor(frame_lens)
    if t.device.type != "cpu":
        t = t.cpu()
    if t.dim() != 1 or t.shape[0] != B or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"frame_lens must be {B} integers (one per row), got {tuple(t.shape)} {t.dtype}")
    if B and (int(t.min()) < 1 or int(t.max()) > T40):
        raise ValueError(f"frame_lens must lie in [1, {T40}] (the padded width), got {t.tolist()}")
    return [int(v) for v in t.tolist()]


SPEED_RANGE = (0.25, 4.0)  # speaking rate r_b: a predicted duration becomes max(1, rint(dsum / r_b))
PITCH_RANGE = (-24.0, 24.0)  # pitch shift p_b in semitones: F0[b, :] *= float32(2 ** (p_b / 12))


def check_row_values(v, B: int, name: str, lo=None, hi=None) -> torch.Tensor:
    """host-side check of one per-request control -> fp32 [B] host tensor.  v: a scalar (broadcast over the rows), a
    sequence or a host tensor of B numbers, each finite and in [lo, hi] where a bound is given; anything else raises
    ValueError (as check_text_lens: a device tensor is never read back)."""
    try:
        t = torch.as_tensor(v)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{name} must be a number or {B} numbers (one per row): {e}")
    if t.device.type != "cpu":
        raise ValueError(f"{name} takes host values")
    if t.dtype == torch.bool or t.is_complex():
        raise ValueError(f"{name} must be real numbers, got {t.dtype}")
    t = t.to(torch.float64)
    if t.dim() == 0:
        t = t.expand(B).clone()
    if t.dim() != 1 or t.shape[0] != B:
        raise ValueError(f"{name} must be a number or {B} numbers (one per row), got shape {tuple(t.shape)}")
    if B and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} must be finite, got {t.tolist()}")
    if B and ((lo is not None and float(t.min()) < lo) or (hi is not None and float(t.max()) > hi)):
        raise ValueError(f"{name} must lie in [{lo}, {hi}], got {t.tolist()}")
    return t.to(torch.float32)


def pitch_factors(pitch_shift: torch.Tensor) -> torch.Tensor:
    """semitones (host fp32 [B]) -> the F0 factors float32(2.0 ** (p / 12)), the power in float64 on the host"""
    return torch.tensor([2.0 ** (float(p) / 12.0) for p in pitch_shift.tolist()], dtype=torch.float64).to(torch.float32)


class RowControls:
    """per-request controls of one batch of B rows (StyleTTSZS.row_controls makes them): guidance
    scale, speaking rate and pitch shift, each optional, each one fp32 [B] device array owned by this object and
    uploaded once.  Row b of a batch run with them computes what the row computes alone with its values as scalars.
    What a batch launches is fixed when the object is made, from the host values:
      cfg_scale   absent, or a scalar: the scalar path as before (`cfg_scalar`, a launch argument).  B values: the CFG
                  form (2B rows, stzs_cfg_euler_rows on `cfg`) when any differs from 1 (`cfg_form`), else the plain form;
      speed       `rate` goes to the durations kernel when any value differs from 1 (`use_rate`);
      pitch_shift `mul` = float32(2 ** (p / 12)) multiplies F0 in one stzs_row_scale launch when any value differs from
                  0 (`use_pitch`).
    A control that is absent or neutral everywhere adds no launch and no argument: the batch is the one without it.
    set() rewrites the arrays in place -- same addresses, no allocation -- so a captured graph replays with the new
    values; a change of what is launched raises ValueError."""

    def __init__(self, B: int, device, cfg_scale=None, speed=None, pitch_shift=None):
        self.B, self.device = int(B), device
        if self.B < 1:
            raise ValueError(f"row_controls: B must be >= 1, got {B}")
        self.cfg_scalar = None
        self.cfg = self.rate = self.mul = None
        self.host = {}
        cfg, rate, pitch = self._check(cfg_scale, speed, pitch_shift)
        if cfg_scale is not None and cfg is None:
            self.cfg_scalar = float(cfg_scale)
        self.cfg_form = cfg is not None and bool((cfg != 1).any())
        self.use_rate = rate is not None and bool((rate != 1).any())
        self.use_pitch = pitch is not None and bool((pitch != 0).any())
        mk = lambda t: None if t is None else torch.empty(self.B, dtype=torch.float32, device=device)
        self.cfg, self.rate, self.mul = mk(cfg), mk(rate), mk(pitch)
        self._upload(cfg, rate, pitch)

    def _check(self, cfg_scale, speed, pitch_shift):
        """-> (cfg | None, rate | None, pitch | None) host fp32 [B]; a scalar cfg_scale is checked and gives None"""
        B = self.B
        cfg = None
        if cfg_scale is not None:
            cfg = check_row_values(cfg_scale, B, "cfg_scale", 0.0)
            if torch.as_tensor(cfg_scale).dim() == 0:
                cfg = None
        rate = None if speed is None else check_row_values(speed, B, "speed", *SPEED_RANGE)
        pitch = None if pitch_shift is None else check_row_values(pitch_shift, B, "pitch_shift", *PITCH_RANGE)
        return cfg, rate, pitch

    def _upload(self, cfg, rate, pitch):
        for name, dst, t in (("cfg_scale", self.cfg, cfg), ("speed", self.rate, rate),
                             ("pitch_shift", self.mul, pitch_factors(pitch) if pitch is not None else None)):
            if t is not None:
                dst.copy_(t)
                self.host[name] = (pitch if name == "pitch_shift" else t).clone()

    def set(self, cfg_scale=None, speed=None, pitch_shift=None):
        """new values for the controls this object was made with, into the same device arrays (a captured graph that
        reads them replays with the new values).  ValueError -- before anything is written -- for a value
        row_controls() would refuse and for a structural change: a control absent when the object was made (or a
        scalar cfg_scale, a launch argument), the CFG form switching on or off, a rate or a pitch shift that was
        neutral everywhere (no launch reads its array) becoming active.  An active rate or pitch may go back to
        neutral: rate 1 and factor 1.0 give the bits of the launch without them."""
        cfg, rate, pitch = self._check(cfg_scale, speed, pitch_shift)
        for name, given, dst in (("cfg_scale", cfg_scale, self.cfg), ("speed", speed, self.rate),
                                 ("pitch_shift", pitch_shift, self.mul)):
            if given is not None and dst is None:
                raise ValueError(f"RowControls.set: {name} was not given per row when the controls were made "
                                 "(structural: make new controls)")
        if cfg_scale is not None and cfg is None:
            raise ValueError("RowControls.set: cfg_scale per row cannot become a scalar (structural)")
        if cfg is not None and bool((cfg != 1).any()) != self.cfg_form:
            raise ValueError("RowControls.set: the CFG form (any cfg_scale != 1) cannot switch on or off (structural)")
        if rate is not None and not self.use_rate and bool((rate != 1).any()):
            raise ValueError("RowControls.set: speed was 1 everywhere when the controls were made (structural)")
        if pitch is not None and not self.use_pitch and bool((pitch != 0).any()):
            raise ValueError("RowControls.set: pitch_shift was 0 everywhere when the controls were made (structural)")
        self._upload(cfg, rate, pitch)
        return self

    def rows(self, B: int):
        """these controls for a batch of B rows -> self (ValueError when B is not theirs)"""
        if int(B) != self.B:
            raise ValueError(f"controls were made for {self.B} rows, the batch has {B}")
        return self


def sigma_schedule(spec: Spec, steps: int):
    """Distilled pins 1: [smax, 0], 2: [smax, 0.5, 0]; otherwise Karras(rho) + trailing 0 (a1)."""
    if steps == 1:
        return [spec.sigma_max, 0.0]
    if steps == 2:
        return [spec.sigma_max, 0.5, 0.0]
    lo, hi = spec.sigma_min ** (1 / spec.rho), spec.sigma_max ** (1 / spec.rho)
    return [(hi + i / (steps - 1) * (lo - hi)) ** spec.rho for i in range(steps)] + [0.0]


def edm_coeffs(spec: Spec, sigma: float):
    sd = spec.sigma_data
    return dict(c_in=1.0 / math.sqrt(sigma ** 2 + sd ** 2), c_skip=sd ** 2 / (sigma ** 2 + sd ** 2),
                c_out=sigma * sd / math.sqrt(sigma ** 2 + sd ** 2), c_noise=math.log(sigma) / 4.0)


def fourier_features(spec: Spec, c_noise: float) -> np.ndarray:
    half = spec.dn_fourier // 2
    f = np.exp(-math.log(10000.0) * np.arange(half) / half)
    arg = 1000.0 * c_noise * f
    return np.concatenate([np.cos(arg), np.sin(arg)]).astype(np.float32)


class _StatsRef:
    """InstanceNorm statistics as fp32 (sum, sumsq) partials of `nch` chunks of `chunk_rows` rows, [B][nch][ld][2]
    in `part`, finalised into mean / rstd (stzs_chan_stats_final) only when something needs them: a generic-path
    conv reads the partials in its AdaIN prologue instead (stzs_conv_args.pro_part, the same bits)."""

    def __init__(self, eng, part, ld, nch, T, B, mean, rstd, chunk_rows, lens=None, lens_mul=1):
        self.eng, self.part, self.ld, self.nch, self.T, self.B = eng, part, ld, nch, T, B
        self.mean, self.rstd, self.chunk_rows, self.done = mean, rstd, chunk_rows, False
        self.lens, self.lens_mul = lens, lens_mul  # ragged frames: the rows each utterance's partials cover

    def final_args(self, s):
        """fill s (stzs_stats_args) for the finalise of these partials -> s"""
        s.mean, s.rstd, s.partial = self.mean.data_ptr(), self.rstd.data_ptr(), self.part.data_ptr()
        s.stat_bs, s.B, s.T, s.C, s.eps = self.ld, self.B, self.T, self.ld, 1e-5
        if self.lens is not None:
            s.lens, s.lens_mul = self.lens.data_ptr(), self.lens_mul
        return s

    def finalize(self):
        if not self.done:
            self.eng._raw(self.eng.lib.stzs_chan_stats_final, "chan_stats_final",
                          C.byref(self.final_args(L.StatsArgs())), self.chunk_rows)
            self.done = True

    def mean_ptr(self):
        self.finalize()
        return self.mean.data_ptr()

    def rstd_ptr(self):
        self.finalize()
        return self.rstd.data_ptr()


class _StatPtr:
    """the mean (which 0) or rstd (1) of a _StatsRef, usable wherever a tensor's data_ptr() is taken (finalises)."""

    def __init__(self, ref, which):
        self.ref, self.which = ref, which

    def data_ptr(self):
        return self.ref.mean_ptr() if self.which == 0 else self.ref.rstd_ptr()

    def tensor(self):
        self.ref.finalize()
        return self.ref.mean if self.which == 0 else self.ref.rstd

    def clone(self):
        return self.tensor().clone()

    def __getitem__(self, k):
        return self.tensor()[k]


class StyleTTSZS:
    def __init__(self, spec: Spec, params, device="cuda:0", fill=True, fp8_denoiser=False, precise_decoder=False,
                 packed: PackedModel = None, branch_streams=False, precise=False, dn_splitk=None, dn_rows=None,
                 te_splitk=None, blk_splitk=None, dur_overlap=None, precise_frontend=False):
        """packed: an already packed (e.g. RCCL-broadcast, stzs/dist.py) PackedModel on `device`; params unused.
        fp8_denoiser: run the per-layer denoiser linears (qkv, o, q, co, ff1, ff2) on e4m3fn MFMA with
        per-row activation / per-column weight scales (configs[4]); bf16 otherwise.
        precise_decoder: PARITY mode for the decoder -- pre-blocks, generator and conv_post keep fp32 activations
        and run every conv on split bf16 operands (hi*hi + hi*lo + lo*hi, STZS_CONV_W_X3, csrc/conv.hip conv_x3).
        precise: the whole pipeline in that mode -- text encoder, style diffusion and prosody predictor too (fp32
        activations, split-operand convs / linears / LSTM recurrences, fp32 attention, libm activations) -- the
        mode that meets the north-star log-mel L1 <= 1e-3 END TO END vs the fp32 oracle (tools/precision_probe.py:
        2.2e-4 in emulation); bf16 weights/activations alone cost ~5e-2.  The reference-prompt
        front end stays bf16: its output is quantised to discrete codes (precise_frontend=True makes it precise too).
        precise_frontend: the reference-prompt front end in fp32, with any of the modes above -- the log-mel in one
        launch (stzs_stft_logmel, csrc/stftmel.hip: fp32 FFT in LDS instead of the bf16 DFT GEMM), the prompt encoder's
        convs, pooling and projection on fp32 activations and split bf16 operands.  The pre-quantiser features then
        match the fp32 oracle to ~1e-5 (the bf16 front end flips ~0.6 % of the discrete codes), so synth() can be
        compared with the oracle from the same reference wav with no code teacher-forced.
        branch_streams: run the independent branches (text encoder || prompt encoder, F0 || N predictor branches)
        on forked side streams (graph-capturable: the fork/join is stream-ordered); each branch has its own
        scratch (statistics slab / workspace), results bit-identical to the single-stream order.
        dur_overlap: with durations given, the alignment reads them directly and the duration LSTM runs in ONE
        launch with the shared F0/N LSTM (stzs_lstm_pair), its projection and durations kernel after the F0/N
        branches -- bit-identical (default on; env STZS_DUR_OVERLAP=0 turns it off)."""
        self.spec = spec
        self.fp8_denoiser = fp8_denoiser
        precise_decoder = precise_decoder or precise
        self.precise = precise_decoder
        self.precise_all = precise
        # precise + fp8_denoiser: the configs[4] long-form mode -- the style sampler on the fp8 denoiser (bf16
        # activations), text encoder / prosody predictor / decoder precise (the F0 phase the harmonic source
        # integrates over 30 s needs the predictor's fp32-level F0: DESIGN.md §3)
        self.lowp_dn = bool(precise and fp8_denoiser)
        self.precise_frontend = bool(precise_frontend)
        self.dec_dt = torch.float32 if precise_decoder else torch.bfloat16
        self.adt = torch.float32 if precise else torch.bfloat16  # text / predictor activations
        self.sdt = torch.bfloat16 if self.lowp_dn else self.adt  # style-sampler activations
        self.device = torch.device(device)
        self.lib = L.load()
        L.check(self.lib.stzs_init(self.device.index or 0), "stzs_init")
        if packed is not None:
            assert packed.spec == spec and packed.arena.buf.device == self.device and \
                packed.precise == precise_decoder and packed.precise_all == precise and \
                getattr(packed, "lowp_denoiser", False) == self.lowp_dn and \
                getattr(packed, "precise_frontend", False) == self.precise_frontend, \
                "packed model: spec / device / precise mode differ"
            self.W = packed
        else:
            self.W = PackedModel(spec, params, self.device, fill=fill, precise=precise_decoder, precise_all=precise,
                                 lowp_denoiser=self.lowp_dn, precise_frontend=self.precise_frontend)
        self._bufs = {}
        self._retired = []
        self._consts = {}
        self.branch_streams = branch_streams
        self._branch = ""  # scratch-key suffix of the branch being enqueued (see fork())
        self._side = {}  # (fork depth, branch) -> side stream
        self._depth = 0  # nesting depth of fork() calls being enqueued
        self.launches = 0
        self.lstm_spin_limit = 0  # 0 = the library default; tests force tiny values
        given = dict(dn_splitk=dn_splitk, dn_rows=dn_rows, te_splitk=te_splitk, blk_splitk=blk_splitk,
                     dur_overlap=dur_overlap)
        for attr, env, default, parse in _KNOBS:
            v = given.get(attr)
            if v is None:
                v = os.environ.get(env, default(self) if callable(default) else default)
            setattr(self, attr, parse(v))
        # device status word collecting the LSTM exchange's spin-timeout flag over every launch (eager or
        # graph-replayed); check_status() reads it and raises
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.prompt_idx = None  # discrete prompt codes of the last prompt_encode (device int32 [B, L_s, G])
        self.frame_lens = None  # frame counts of the last synth_stream(ragged_frames=True) (device int32 [B])

    def row_controls(self, B: int, cfg_scale=None, speed=None, pitch_shift=None) -> RowControls:
        """per-request controls for a batch of B rows (RowControls).  Each of cfg_scale (>= 0; 0 is the
        pure unconditional sample), speed (SPEED_RANGE) and pitch_shift (semitones, PITCH_RANGE) is None, a scalar, a
        list or a host tensor of B values; wrong shapes, non-finite and out-of-range values raise ValueError.  The
        values are uploaded once into device arrays the result owns; hand it to sample_style / predict_durations /
        predict_prosody / prosody_frames / f0n_predictor / synth / synth_stream as controls=."""
        return RowControls(B, self.device, cfg_scale, speed, pitch_shift)

    def check_status(self, reset=True):
        """raise RuntimeError if any LSTM exchange since the last check timed out (its h-states are wrong).
        Synchronizes the device (one 4-B copy)."""
        v = int(self.status.item())
        if reset and v:
            self.status.zero_()
        if v & L.STATUS_LSTM_TIMEOUT:
            raise RuntimeError("stzs_lstm: exchange spin timed out (LSTM workgroups not co-resident?); "
                               "the prosody outputs of this call are invalid")
        return v

    @classmethod
    def from_checkpoint(cls, path: str, device="cuda:0", **kw) -> "StyleTTSZS":
        """engine on the parameters of a safetensors checkpoint (stzs/checkpoint.py), spec from its metadata."""
        from .checkpoint import load_params
        params, spec = load_params(path)
        return cls(spec, params, device=device, **kw)

    # ------------------------------------------------------------------ plumbing
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def buf(self, key, shape, dtype=torch.bfloat16, zero=False):
        """cached device buffer: ONE storage per (key, dtype), reused by capacity for every shape that fits, so a
        stream of distinct request lengths (stzs/scheduler.py) does not allocate a buffer set per length.  The
        address is stable while the shape fits (graph-capturable); a shape change re-zeroes zero=True buffers
        (their padding rows / channels are read by the kernels); growth allocates 1.25x the request and keeps
        the old storage alive in self._retired, so graphs captured on it stay valid."""
        k = (key, dtype)
        shape = tuple(int(v) for v in shape)
        n = 1
        for v in shape:
            n *= v
        ent = self._bufs.get(k)
        # a storage a captured graph reads (ent[3], set by capture()) is never re-viewed at another shape:
        # the graph would replay over the other shape's data and padding
        if ent is None or ent[0].numel() < n or (ent[3] and ent[1] != shape):
            if ent is not None:
                self._retired.append(ent[0])
            cap = n if ent is None else max(n, int(ent[0].numel() * 1.25))
            store = torch.zeros(max(cap, 1), dtype=dtype, device=self.device) if zero else \
                torch.empty(max(cap, 1), dtype=dtype, device=self.device)
            ent = self._bufs[k] = [store, shape, store[:n].view(shape), False]
            return ent[2]
        if ent[1] != shape:
            ent[1] = shape
            ent[2] = ent[0][:n].view(shape)
            if zero:
                ent[2].zero_()
        return ent[2]

    def buffer_bytes(self) -> int:
        """device bytes held by the buffer cache (live storages + retired ones kept for captured graphs)."""
        live = sum(e[0].numel() * e[0].element_size() for k, e in self._bufs.items() if isinstance(k, tuple))
        return live + sum(t.numel() * t.element_size() for t in self._retired)

    def act(self, key, B, T, C, dtype=torch.bfloat16):
        return Act(self.buf(key, (B, T, _rup(C, 8)), dtype, zero=True), 0, C)

    def _t(self, x):
        """weight reference -> device tensor (arena name, or an already-resolved tensor)."""
        return x if isinstance(x, torch.Tensor) else self.W.t(x)

    def _call(self, fn, arg, what, cost=None, b=None, shape=None, args=None):
        """one library launch: counted, its result checked, and timed here and nowhere else (but for _launch_group,
        whose call returns its own launch count, and the span query of _istft_chunk, no launch).  b: a second struct
        argument (stzs_lstm_pair); args: the whole argument list (without the stream) when it is not one or two
        structs.  cost = (algorithmic FLOP, algorithmic bytes) of it, or a function giving them, evaluated only when
        the launch is recorded with HIP events: a conv (shape = (ks, dil, T_out, Co)) under a timer of every launch
        or of its tag, any other launch with a cost under a timer of every launch (start_timer("*"), the per-stage
        roofline of bench.py)."""
        self.launches += 1
        if args is None:
            args = (C.byref(arg),) if b is None else (C.byref(arg), C.byref(b))
        tm = self.timer
        rec = tm is not None and ((tm["all"] or what in tm["tags"]) if shape is not None else
                                  (tm["all"] and cost is not None))
        if rec:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
        L.check(fn(*args, self.stream()), what)
        if rec:
            e1.record()
            # (a cost function's figures are recorded as they come, a given pair as floats)
            flop, byt = cost() if callable(cost) else (float(cost[0]), float(cost[1]))
            tm["rec"].append((what, e0, e1, flop, byt, shape, self.stage))

    def _raw(self, fn, what, *args):
        """a launch whose arguments are not one struct (plain pointers and sizes, a struct array): never timed"""
        self._call(fn, None, what, args=args)

    # ------------------------------------------------------------------ ops
    def conv(self, cw: ConvW, x: Act, y: Act, *, T_out=None, pad=0, dil=1, stride=1, pro=None, pro_act=L.ACT_NONE,
             pro_slope=0.0, pro_alpha=None, cscale=1.0, res: Act = None, res_tdiv=1, acc_in: Act = None,
             alpha=1.0, beta=0.0, gate=None, gate_bs=0, epi_act=L.ACT_NONE, epi_slope=0.0, ups_pad=0,
             T_final=0, refl=0, flags=0, stats_key=None, x_scale=None, post_ln=None, pre_ln=None, splitk=0, rows=0,
             attn=None, collect=None, t_lens=None, t_lens_mul=1, t_lens_rows=0, what="conv"):
        """-> y, or (y, (mean, rstd, stat_bs)) with stats_key: InstanceNorm statistics of the stored
        output fused into the conv epilogue (per-tile partials) + one small finalize launch.
        collect (a list): append the conv's stzs_conv_args to it instead of launching (the caller launches the
        collected problems with stzs_conv1d_group, and finalises their statistics -- returned unfinalised, per-key
        slabs -- with _finalize_group).
        post_ln (stzs_rowln_args) / attn ((q, k, v, o) Acts): the LayerNorm / attention that consumes y, launched
        behind the linear.  (r03 also ran them, and the sampler's CFG + Euler step, inside the small-M linear's launch
        by its last-arriving workgroups: bit-identical but slower at batch 1, removed in r04 -- DESIGN.md §5.)
        pre_ln (stzs_rowln_args): the LayerNorm whose output x is, launched before the linear -- or, on the small-M
        rows form, fused into it (stzs_ln_linear, csrc/lnrows.hip: the normalised rows never leave the chip).
        t_lens (int32 [B] device tensor, ragged frames): utterance b holds t_lens[b] * t_lens_mul rows
        (stzs_conv_args.t_lens; the library refuses the forms that do not honour it); its fused statistics are
        finalised here with the same lengths, never deferred.  t_lens_rows=1 (the ragged decoder): t_lens[b] is the
        utterance's own row count on this conv's input time axis (stzs_conv_args.t_lens_rows)."""
        a, pro_ref = self._conv_fill(cw, x, y, what, T_out=T_out, pad=pad, dil=dil, stride=stride, pro=pro,
                                     pro_act=pro_act, pro_slope=pro_slope, pro_alpha=pro_alpha, cscale=cscale, res=res,
                                     res_tdiv=res_tdiv, acc_in=acc_in, alpha=alpha, beta=beta, gate=gate,
                                     gate_bs=gate_bs, epi_act=epi_act, epi_slope=epi_slope, ups_pad=ups_pad,
                                     T_final=T_final, refl=refl, x_scale=x_scale)
        rows = self._conv_route(a, cw, x, y, flags, rows, cscale, res, stats_key)
        if t_lens is not None:
            assert collect is None and pro_ref is None and splitk <= 1 and rows == 0, what
            a.t_lens, a.t_lens_mul, a.t_lens_rows = t_lens.data_ptr(), t_lens_mul, t_lens_rows
        if rows > 1 or splitk > 1:
            self._conv_splitk(a, cw, x, splitk, rows, collect, what)
        if pro_ref is not None:
            self._conv_stats_in(a, cw, pro_ref, pre_ln)
        st = self._conv_stats_out(a, cw, y, stats_key, collect, t_lens is not None) if stats_key is not None else None
        fn, args, fused = self._conv_entry(a, cw, x, res, res_tdiv, gate, pre_ln, st)
        if collect is not None:
            assert len(args) == 1 and pre_ln is None and post_ln is None and attn is None, what
            collect.append(a)
        else:
            if pre_ln is not None and not fused:
                self._call(self.lib.stzs_row_layernorm, pre_ln, what + ".ln", cost=_ln_cost(pre_ln))
            # (its shape and cost model are needed only for a record)
            rec = {} if self.timer is None else dict(
                shape=(cw.ks, dil, a.T_out, cw.Co),
                cost=partial(_conv_cost, cw, x, y, a.T_out, res, acc_in, pre_ln if fused else None))
            self._call(fn, a, what, args=args, **rec)
        if post_ln is not None:  # the LayerNorm that consumes this linear's output (stzs_rowln_args)
            self._call(self.lib.stzs_row_layernorm, post_ln, what + ".ln", cost=_ln_cost(post_ln))
        if attn is not None:  # the attention whose q (k, v) this linear produced
            self.attention(*attn)
        if st is None:
            return y
        slab, Cc, mean, rstd, defer, ntile = st
        ref = _StatsRef(self, slab, Cc, ntile, a.T_out, y.B, mean, rstd, L.CONV_STAT_ROWS, t_lens, t_lens_mul)
        if not defer:
            ref.finalize()
            return y, (mean, rstd, Cc)
        return y, (_StatPtr(ref, 0), _StatPtr(ref, 1), Cc)

    def _conv_fill(self, cw, x, y, what, *, T_out, pad, dil, stride, pro, pro_act, pro_slope, pro_alpha, cscale, res,
                   res_tdiv, acc_in, alpha, beta, gate, gate_bs, epi_act, epi_slope, ups_pad, T_final, refl, x_scale):
        """conv() step 1 (conv()'s own arguments, by name): the problem as stzs_conv_args -- weight form, workspaces
        and statistics not yet chosen
        -> (args, the deferred statistics of the AdaIN prologue still to be resolved | None)"""
        a = L.ConvArgs()
        a.x, a.w, a.y = x.ptr, self._t(cw.w).data_ptr(), y.ptr
        a.bias = self._t(cw.b).data_ptr() if cw.b is not None else None
        a.ldx, a.bsx, a.ldy, a.bsy = x.ld, x.bs, y.ld, y.bs
        T = x.T
        a.B, a.T_in, a.Ci, a.Co, a.ks, a.dil, a.stride, a.pad = x.B, T, cw.Ci, cw.Co, cw.ks, dil, stride, pad
        assert x.C == cw.Ci, (what, x.C, cw.Ci)
        if cw.ups:
            a.T_out = T + 1
            a.ups, a.ups_pad, a.T_final, a.refl = cw.ups, ups_pad, T_final, refl
            a.pad = 1
        else:
            a.T_out = T_out if T_out is not None else (T + 2 * pad - dil * (cw.ks - 1) - 1) // stride + 1
        a.ci_pad, a.co_pad, a.cic = cw.ci_pad, cw.co_pad, cw.cic
        a.in_dtype, a.out_dtype = x.dt, y.dt
        pro_ref = None
        if pro is not None:  # AdaIN: (mean, rstd, stat_bs, gb_ptr, gb_bs, beta_off)
            mean, rstd, stat_bs, gbp, gb_bs, boff = pro
            a.pro_mode = L.PRO_ADAIN
            if isinstance(mean, _StatPtr) and not mean.ref.done:
                pro_ref = mean.ref  # (resolved by _conv_stats_in, once the path is known)
            else:
                a.pro_mean, a.pro_rstd = mean.data_ptr(), rstd.data_ptr()
            a.stat_bs = stat_bs
            a.pro_gb, a.gb_bs, a.gb_beta_off = gbp, gb_bs, boff
        a.pro_act, a.pro_slope, a.pro_cscale = pro_act, pro_slope, cscale
        a.pro_alpha = self._t(pro_alpha).data_ptr() if pro_alpha is not None else None
        if res is not None:
            assert res.t.dtype == y.t.dtype
            a.res, a.ldr, a.bsr = res.ptr, res.ld, (res.bs if res.B > 1 or res.B == y.B else 0)
        a.res_tdiv = res_tdiv
        if acc_in is not None:
            a.acc_in, a.lda, a.bsa = acc_in.ptr, acc_in.ld, acc_in.bs
        if gate is not None:
            a.gate, a.gate_bs = gate, gate_bs
        a.alpha, a.beta, a.epi_act, a.epi_slope = alpha, beta, epi_act, epi_slope
        if cw.f8:
            assert x.t.dtype == torch.float8_e4m3fn and x_scale is not None, what
            a.x_scale, a.w_scale = x_scale.data_ptr(), self._t(cw.wscale).data_ptr()
        return a, pro_ref

    def _conv_route(self, a, cw, x, y, flags, rows, cscale, res, stats_key) -> int:
        """conv() step 2: the kernel form of the filled problem a -- sets a.flags, and a.w / a.cic where the form has
        a weight copy of its own.  rows: the K slices asked of the small-M rows form -> those it takes (0: not on it).
        Beside a it takes what a does not hold exactly: the Acts, cscale as given (a's is rounded to fp32), and
        whether statistics are asked for."""
        T_out, xT, xdt = a.T_out, x.T, x.t.dtype
        stride, pad, pro_act, epi_act, res_tdiv = a.stride, a.pad, a.pro_act, a.epi_act, a.res_tdiv  # (pad 1 with ups)
        no_pro, no_gate, no_acc = a.pro_mode == L.PRO_NONE, not a.gate, not a.acc_in
        bare = no_pro and pro_act == L.ACT_NONE  # no prologue
        # a plain linear: row for row, no prologue, every row readable over ci_pad channels
        plain = (cw.ks == 1 and stride == 1 and pad == 0 and not cw.ups and bare and x.c0 + cw.ci_pad <= x.ld and
                 T_out == xT)
        if (plain and not getattr(cw, "frag32", False)  # (the 1x1 block shortcuts on the register-direct form)
                and cscale == 1.0 and xdt in (torch.bfloat16, torch.float8_e4m3fn)):
            flags |= 8  # STZS_CONV_A_DMA: the LDS-DMA GEMM path
        fx3_conv = (cw.ks in (3, 7, 11) and epi_act == L.ACT_NONE and no_gate and
                    (pro_act == L.ACT_SNAKE or (cw.ks == 3 and no_acc) or
                     (cw.Co <= 32 and cw.ks == 7 and pro_act == L.ACT_LEAKY and no_pro and res is None and
                      no_acc and stats_key is None)))  # (the last: conv_post on the narrow form)
        fx3_lin = (cw.ks == 1 and pad == 0 and bare and stats_key is None and
                   T_out == xT and epi_act in (L.ACT_NONE, L.ACT_GELU, L.ACT_SILU) and res_tdiv == 1)
        if (getattr(cw, "fx3", None) is not None and self.mrfx and xdt == torch.float32 and
                y.t.dtype == torch.float32 and stride == 1 and not cw.ups and (fx3_conv or fx3_lin) and
                (res is None or res.t.dtype == torch.float32) and x.ptr % 32 == 0 and y.ptr % 32 == 0):
            # precise mode, register-direct: split bf16 operands on the mrfv data movement (csrc/mrfx.hip; the linears
            # on its FLAT form mrfx_lin)
            a.w, a.cic = self._t(cw.fx3).data_ptr(), 128
            flags = (flags & ~8) | L.CONV_W_FRAG32X3
        elif cw.wx3 is not None:  # precise mode: split bf16 operands (csrc/conv.hip conv_x3)
            a.w, a.cic = self._t(cw.wx3).data_ptr(), 32
            flags = (flags & ~8) | L.CONV_W_X3
        elif cw.w32 is not None:  # fp32 operands on fp32 MFMA (csrc/conv.hip conv_f32)
            a.w, a.cic = self._t(cw.w32).data_ptr(), 32
            flags = (flags & ~8) | L.CONV_W_F32
        elif getattr(cw, "frag32", False):
            flags |= L.CONV_W_FRAG32  # register-direct MRF kernel (csrc/mrfv.hip)
        elif getattr(cw, "lane16", False):
            flags |= L.CONV_W_LANE16  # MRF-family kernel (csrc/mrf.hip)
        elif getattr(cw, "narrow32", False):
            flags |= L.CONV_W_NARROW32  # narrow conv (csrc/mrf.hip)
        a.flags = flags | self.conv_flags
        nk = cw.ci_pad // 32
        if rows > 0 and not (nk % (4 * rows) == 0 and nk // (4 * rows) in (1, 2, 4, 8, 16)):
            rows = 0  # (a function of K only: batch invariance holds)
        if not (rows > 0 and plain and not cw.f8 and cw.wx3 is None and cw.w32 is None and stats_key is None and
                (xdt == torch.float32 or (xdt == torch.bfloat16 and cscale == 1.0)) and
                epi_act in (L.ACT_NONE, L.ACT_GELU, L.ACT_SILU)):
            return 0
        # small-M linear on the whole chip (csrc/rows.hip): 16-column tiles x K split in `rows` slices
        a.flags = (a.flags & ~8) | L.CONV_ROWS
        return rows

    def _conv_splitk(self, a, cw, x, splitk, rows, collect, what):
        """conv() step 3: the K slices of a (a.splitk) with their fp32 slabs and hand-off counters, by its form: the
        rows form's `rows` (from _conv_route), else up to `splitk` on the LDS-DMA GEMM or the generic path."""
        if rows > 0:
            if rows > 1:
                a.splitk = rows
                nb = self.lib.stzs_conv_rows_workspace(x.B * x.T, cw.Co, rows)
                a.splitk_ws = self._scratch("rows_ws", nb // 4 + 1).data_ptr()
                a.splitk_ctr = self._counters("rows_ctr", nb // (rows * 16)).data_ptr()
            return
        if a.flags & 8:  # LDS-DMA GEMM: the slices split the K-steps (a function of K only: batch invariance holds)
            splitk = min(splitk, 4)  # (gemm_glds takes 2 or 4 slices)
            while splitk > 1 and (cw.ci_pad // 32) % splitk:
                splitk //= 2
        elif splitk > 1:  # conv_mfma: the slices split the input-channel chunks (2..16, at most one slice per chunk;
            # one chunk per slice takes the DEEP form: the slice's whole weight stream issued at entry)
            splitk = min(splitk, 16, cw.ci_pad // cw.cic)
        if splitk > 1 and (a.flags & 8) and not cw.f8 and cw.wx3 is None and cw.w32 is None:
            # in-launch split-K (stzs_conv_args.splitk): per-branch fp32 slabs + self-resetting tile counters
            nb = self.lib.stzs_conv_splitk_workspace(x.B * x.T, cw.co_pad, splitk)
            assert nb > 0, (what, splitk)
            a.splitk, a.splitk_ws = splitk, self._scratch("sk_ws", nb // 4).data_ptr()
            a.splitk_ctr = self._counters("sk_ctr", nb // (splitk * 32768)).data_ptr()
        elif splitk > 1 and _conv_generic(a.flags, cw):
            # conv_mfma split over input-channel chunks: one 64-KB fp32 slab per (128-row tile, slice) + a ticket
            # per tile (grid.x is at most B x ceil(T_out / 128))
            tiles = x.B * ((a.T_out + 127) // 128) * (cw.co_pad // 128)
            a.splitk = splitk
            gs = f".g{len(collect)}" if collect is not None else ""  # (a collected problem: its own slabs)
            a.splitk_ws = self._scratch("csk_ws" + gs, tiles * splitk * 16384).data_ptr()
            a.splitk_ctr = self._counters("csk_ctr" + gs, tiles).data_ptr()

    def _conv_stats_in(self, a, cw, pro_ref, pre_ln):
        """conv() step 4: the AdaIN prologue's statistics when they are still partials (pro_ref, a _StatsRef)"""
        if _conv_generic(a.flags, cw) and pre_ln is None and pro_ref.nch <= 8:
            # the prologue finalises the partials itself
            a.pro_part, a.pro_ld, a.pro_nch, a.pro_T, a.pro_eps = pro_ref.part.data_ptr(), pro_ref.ld, pro_ref.nch, \
                pro_ref.T, 1e-5
        else:
            a.pro_mean, a.pro_rstd = pro_ref.mean_ptr(), pro_ref.rstd_ptr()

    def _conv_stats_out(self, a, cw, y, stats_key, collect, ragged=False):
        """conv() step 5: the slab the epilogue writes the output's statistics partials to, and their mean / rstd
        buffers -> (slab, channels, mean, rstd, finalise deferred?, partial chunks)"""
        Cc = _rup(cw.Co, 8)
        ntile = (a.T_out + L.CONV_STAT_ROWS - 1) // L.CONV_STAT_ROWS
        defer = (collect is not None or (self.defer_stats and ntile <= 8)) and not ragged
        # (deferred: the partials must outlive this launch until their consumer reads them -- a slab per key)
        slab = self._scratch("stat_slab." + stats_key, y.B * ntile * Cc * 2, 1024) if defer else \
            self._scratch("stat_slab", y.B * ntile * Cc * 2)
        a.stat_part, a.stat_ld = slab.data_ptr(), Cc
        return (slab, Cc, self.buf(stats_key + ".m", (y.B, Cc), torch.float32),
                self.buf(stats_key + ".r", (y.B, Cc), torch.float32), defer, ntile)

    def _conv_entry(self, a, cw, x, res, res_tdiv, gate, pre_ln, st):
        """conv() step 6: the library entry point of a -> (function, its arguments, pre_ln fused into the launch?):
        stzs_conv1d, or for a rows-form linear stzs_ln_linear, with the LayerNorm pre_ln in front or as the 16-row
        form (ln = NULL)."""
        if not (a.flags & L.CONV_ROWS):
            return self.lib.stzs_conv1d, (C.byref(a),), False
        nk = cw.ci_pad // 32
        if pre_ln is not None:
            fused = a.splitk <= 1 and res is None and gate is None and \
                st is None and pre_ln.C == cw.Ci == cw.ci_pad and nk in (4, 8, 16) and pre_ln.out_dtype == L.BF16 and \
                pre_ln.act == L.ACT_NONE and (pre_ln.x or 0) % 16 == 0 and pre_ln.ldx % 8 == 0 and \
                pre_ln.gdiv > 0 and pre_ln.R < (1 << 22) - 16 and \
                (not pre_ln.G or (pre_ln.gs % 8 == 0 and pre_ln.G % 32 == 0)) and \
                (not pre_ln.Bt or (pre_ln.bs % 8 == 0 and pre_ln.Bt % 32 == 0))
            # (every condition stzs_ln_linear checks, csrc/lnrows.hip: a shape it refuses takes the two launches)
            if fused:
                return self.lib.stzs_ln_linear, (C.byref(a), C.byref(pre_ln)), True
        # a rows-form linear on the 16-row register-direct form (stzs_ln_linear, ln = NULL): K <= rows16_maxk as one
        # sequential chain per element (its K slices dropped), or with its Z in {2, 4} slices of 4..16 K-steps
        r16 = (pre_ln is None and self.rows16 and st is None and
               (res is None or res_tdiv == 1) and x.ptr % 16 == 0 and x.ld % 8 == 0 and x.bs % 8 == 0)
        r16_split = r16 and self.rows16_split and a.splitk in (2, 4) and nk % a.splitk == 0 and \
            nk // a.splitk in (4, 8, 16)
        if r16_split or (r16 and nk in (4, 8, 16, 32, 64) and cw.ci_pad <= self.rows16_maxk):
            if not r16_split:
                a.splitk = 0
            return self.lib.stzs_ln_linear, (C.byref(a), None), False
        return self.lib.stzs_conv1d, (C.byref(a),), False

    def _rows_z(self, cw: ConvW) -> int:
        """1 = the whole-chip small-M form (one K slice: no hand-off state) for a per-utterance linear whose K gives
        every wave the same K-step count, 0 = the tiled path -- a function of the weight's shape only (the native
        composite operators, csrc/abi_ops.hip, apply the same rule: bit-identical)."""
        nk = cw.ci_pad // 32
        return int(self.small_rows and nk % 4 == 0 and nk // 4 in (1, 2, 4, 8, 16))

    def _scratch(self, name, n, minimum=1 << 20):
        """fp32 scratch shared by consecutive launches of ONE branch (a conv's statistics partials, consumed by
        the finalize launch right behind it; the standalone statistics workspace).  Each forked branch has its
        own (key suffix self._branch): concurrent branches sharing one slab would race on the partials.  A
        grown slab's old storage is retired, not freed: launches already enqueued (or captured) on it --
        possibly on another stream -- still read it, and a freed block could be handed to another stream's
        allocation while they run.  minimum: the smallest storage (the shared slabs start at 4 MB so they rarely grow;
        the per-key deferred-statistics slabs are sized exactly -- a batch-1 partial is a few KB)."""
        key = name + self._branch
        t = self._bufs.get(key)
        if t is None or t.numel() < n:
            if t is not None:
                self._retired.append(t)
            t = self._bufs[key] = torch.empty(max(n, minimum), dtype=torch.float32, device=self.device)
        return t

    def _counters(self, name, n):
        """int32 hand-off counters of ONE branch, zero when allocated; every kernel that uses them leaves them zero
        (the split-K tile tickets).  Grown storages are retired, like _scratch."""
        key = name + self._branch
        t = self._bufs.get(key)
        if t is None or t.numel() < n:
            if t is not None:
                self._retired.append(t)
            t = self._bufs[key] = torch.zeros(max(n, 4096), dtype=torch.int32, device=self.device)
        return t

    def _fork_on(self, site) -> bool:
        """branch_streams covers the fork site: True = every site, or a set of site names"""
        bs = self.branch_streams
        return bs is True or (isinstance(bs, (set, frozenset)) and site in bs)

    def fork(self, site, *fns):
        """run fns[0] on the current stream and fns[1:] on side streams forked from it (waits on the current
        stream, joined back into it before returning); sequential unless branch_streams is on (True, or a set of
        fork sites holding `site`: "enc" = text || prompt encoder, "f0n" = F0 || N predictor branches, "src" =
        decoder pre-blocks || harmonic source).
        Forks nest: a fork inside a branch takes side streams and scratch keys of its own depth, so an inner
        branch never queues behind (or shares scratch with) an outer one.  -> outputs"""
        if not self._fork_on(site) or len(fns) < 2:
            return [f() for f in fns]
        cur = torch.cuda.current_stream(self.device)
        d, outer = self._depth, self._branch
        side = []
        for i in range(1, len(fns)):
            if (d, i) not in self._side:
                self._side[(d, i)] = torch.cuda.Stream(self.device)
            side.append(self._side[(d, i)])
        for st in side:
            st.wait_stream(cur)
        outs = []
        self._depth = d + 1
        try:
            for i, f in enumerate(fns):
                self._branch = outer if i == 0 else f"{outer}@b{d}.{i}"
                with torch.cuda.stream(cur if i == 0 else side[i - 1]):
                    outs.append(f())
        finally:
            self._branch, self._depth = outer, d
        for st in side:
            cur.wait_stream(st)
        return outs

    timer = None
    stage = ""  # label of the synth() stage being enqueued (set by the caller; recorded with each timed launch)

    def start_timer(self, tags):
        """record HIP events around every conv launch whose tag is in `tags` (same stream as the kernel); tags "*":
        every conv launch and every other launch whose algorithmic cost the engine models (attention, LSTM
        recurrences, LayerNorm rows, statistics, harmonic source, iSTFT)."""
        self.timer = dict(tags=set(tags) if tags != "*" else set(), all=tags == "*", rec=[])

    def stop_timer(self):
        """-> [(tag, seconds, FLOP, bytes, conv shape | None, stage)] of the recorded launches, in launch order."""
        tm, self.timer = self.timer, None
        torch.cuda.synchronize(self.device)
        return [(w, e0.elapsed_time(e1) * 1e-3, f, b, shp, stg) for (w, e0, e1, f, b, shp, stg) in tm["rec"]]

    def stats(self, x: Act, key, lens=None, lens_mul=1):
        """InstanceNorm statistics of x over time -> (mean, rstd, stat_bs); with defer_stats and <= 8 256-row chunks
        only the partials pass runs here (the consuming conv's prologue, or the first other use, finalises).
        lens (int32 [B] device tensor, ragged frames): over utterance b's first lens[b] * lens_mul rows, finalised
        here."""
        Cc = _rup(x.C, 8)
        mean = self.buf(key + ".m", (x.B, Cc), torch.float32)
        rstd = self.buf(key + ".r", (x.B, Cc), torch.float32)
        nch = (x.T + 255) // 256
        defer = self.defer_stats and nch <= 8 and lens is None
        nws = self.lib.stzs_chan_stats_workspace(x.B, x.T, Cc) // 4 + 1
        ws = self._scratch("stat_ws." + key, nws, 1024) if defer else self._scratch("stat_ws", nws)
        a = L.StatsArgs()
        a.x, a.mean, a.rstd, a.partial = x.ptr, mean.data_ptr(), rstd.data_ptr(), ws.data_ptr()
        a.ld, a.bs, a.stat_bs, a.B, a.T, a.C, a.dtype, a.eps = x.ld, x.bs, Cc, x.B, x.T, Cc, x.dt, 1e-5
        if lens is not None:
            a.lens, a.lens_mul = lens.data_ptr(), lens_mul
        cost = (0, x.B * x.T * x.C * x.t.element_size())
        if not defer:
            self._call(self.lib.stzs_chan_stats, a, "chan_stats", cost=cost)
            return mean, rstd, Cc
        self._call(self.lib.stzs_chan_stats_partial, a, "chan_stats", cost=cost)
        ref = _StatsRef(self, ws, Cc, nch, x.T, x.B, mean, rstd, 256)
        return _StatPtr(ref, 0), _StatPtr(ref, 1), Cc

    def rowln(self, x: Act, y: Act, *, G=None, gs=0, Bt=None, bs=0, gdiv=1, gadd=1.0, act=L.ACT_NONE, slope=0.0,
              R=None, y_scale=None, lens=None, what="rowln"):
        """lens (int32 [B] device tensor): rows t >= lens[b] of the x.T-row blocks are stored as zeros"""
        a = self._ln_args(x, y, G=G, gs=gs, Bt=Bt, bs=bs, gdiv=gdiv, gadd=gadd, y_scale=y_scale)
        a.act, a.slope = act, slope
        if lens is not None:
            a.lens, a.T = lens.data_ptr(), x.T
        if R is not None:
            a.R = R
        assert x.ld * x.T == x.bs and y.ld * y.T == y.bs
        self._call(self.lib.stzs_row_layernorm, a, what, cost=_ln_cost(a))

    def quant(self, x: Act, y: Act, scale: torch.Tensor, what="quant"):
        """bf16 rows -> e4m3fn rows + per-row scale (stzs_quant_rows)."""
        a = L.QuantArgs()
        a.x, a.y, a.scale, a.ldx, a.ldy = x.ptr, y.ptr, scale.data_ptr(), x.ld, y.ld
        a.R, a.C = x.B * x.T, x.C
        assert x.ld * x.T == x.bs and y.ld * y.T == y.bs
        self._call(self.lib.stzs_quant_rows, a, what, cost=(0, a.R * a.C * (x.t.element_size() + 1)))

    def _attn_args(self, q: Act, k: Act, v: Act, o: Act):
        S = self.spec
        a = L.AttnArgs()
        a.q, a.k, a.v, a.o = q.ptr, k.ptr, v.ptr, o.ptr
        a.ldq, a.ldk, a.ldv, a.ldo = q.ld, k.ld, v.ld, o.ld
        a.bsq, a.bsk, a.bsv, a.bso = q.bs, k.bs, v.bs, o.bs
        a.R, a.Lq, a.Lk, a.heads, a.dh = q.B, q.T, k.T, S.dn_heads, S.dn_head_dim
        a.precise = int(q.t.dtype == torch.float32)  # fp32 operands: the fp32 attention kernel
        return a

    def attention(self, q: Act, k: Act, v: Act, o: Act, lk_rows: torch.Tensor = None):
        """lk_rows (int32 [R] device tensor): row r attends to its first lk_rows[r] keys only"""
        a = self._attn_args(q, k, v, o)
        if lk_rows is not None:
            a.lk_rows = lk_rows.data_ptr()
        self._call(self.lib.stzs_attention, a, "attention",
                   cost=(4.0 * a.R * a.heads * a.Lq * a.Lk * a.dh,
                         a.R * (2 * a.Lq + 2 * a.Lk) * a.heads * a.dh * q.t.element_size()))

    def lstm(self, lw, x: Act, y: Act, key, lens: torch.Tensor = None):
        """lens (int32 [B] device tensor): utterance b runs as alone at T = lens[b], y[b, t >= lens[b]] = 0"""
        a, cost = self._lstm_args(lw, x, y, key, lens=lens)
        self._call(self.lib.stzs_lstm, a, key + ".rec", cost=cost)  # recurrent products + gate rows in, h rows out
        return y

    def lstm_pair(self, r0, r1):
        """two independent recurrences r = (lw, x, y, key[, lens]) of one shape class in ONE launch (stzs_lstm_pair:
        side by side on the chip; each output the same bits as its own lstm() call): both input projections, then
        the paired recurrence on separate exchange state."""
        a0, c0 = self._lstm_args(*r0[:4], lens=r0[4] if len(r0) > 4 else None)
        a1, c1 = self._lstm_args(*r1[:4], pair=True, lens=r1[4] if len(r1) > 4 else None)
        self._call(self.lib.stzs_lstm_pair, a0, r0[3] + ".rec+" + r1[3] + ".rec",
                   cost=(c0[0] + c1[0], c0[1] + c1[1]), b=a1)
        return r0[2], r1[2]

    def _lstm_args(self, lw, x: Act, y: Act, key, pair=False, lens=None):
        """input projection (one MFMA GEMM over all steps) + the recurrence's arguments -> (LstmArgs, cost)"""
        gx = self.act(key + ".gx", x.B, x.T, 8 * lw.H, torch.float32)
        self.conv(lw.ih, x, gx, what=key + ".ih")
        a = L.LstmArgs()
        a.gx, a.whhT, a.y = gx.ptr, self._t(lw.whhT).data_ptr(), y.ptr
        if lw.whx3 is not None:  # precise: split-operand recurrence, fp32 h out
            assert y.t.dtype == torch.float32
            a.whhT, a.precise = self._t(lw.whx3).data_ptr(), 1
        nx = self.lib.stzs_lstm_workspace(x.B, lw.H, 2)
        sk = self._branch + ("@pair" if pair else "")  # concurrent recurrences (branches, a pair) never share them
        xchg = self.buf("lstm.xchg" + sk, (max(nx, 16),), torch.uint8, zero=True)
        sync = self.buf("lstm.sync" + sk, (4096,), torch.uint8, zero=True)
        a.xchg, a.sync = xchg.data_ptr(), sync.data_ptr()
        a.ldg, a.bsg, a.ldy, a.bsy = gx.ld, gx.bs, y.ld, y.bs
        a.B, a.T, a.H, a.ndir = x.B, x.T, lw.H, 2
        a.status, a.spin_limit = self.status.data_ptr(), self.lstm_spin_limit
        a.lens = lens.data_ptr() if lens is not None else None
        # (flops, bytes): recurrent products; gate rows in, h rows out, W_hh once
        return a, (2.0 * x.B * x.T * 2 * 4 * lw.H * lw.H,
                   x.B * x.T * (8 * lw.H * 4 + 2 * lw.H * y.t.element_size()) + 2 * 4 * lw.H * lw.H * 2)

    def copy2d(self, x: Act, y: Act, R, Cn, bsx=None):
        self._copy_rows(x.ptr, x.ld, x.bs if bsx is None else bsx, y.ptr, y.ld, y.bs, y.B, R, Cn, x.dt, y.dt, "copy2d")

    def _copy_rows(self, x: int, ldx: int, bsx: int, y: int, ldy: int, bsy: int, nb: int, R: int, Cn: int, dti, dto,
                   what="copy_windows", row_off: torch.Tensor = None):
        """stzs_copy2d on raw byte addresses: nb blocks of R rows x Cn columns (source block stride bsx elements);
        row_off (int32 [nb] device tensor): block b lands row_off[b] rows further down in y"""
        a = L.CopyArgs()
        a.dst_row_off = row_off.data_ptr() if row_off is not None else None
        a.x, a.y, a.ldx, a.bsx, a.ldy, a.bsy = x, y, ldx, bsx, ldy, bsy
        a.B, a.R, a.C, a.in_dtype, a.out_dtype = nb, R, Cn, dti, dto
        self._call(self.lib.stzs_copy2d, a, what)

    def mean_rows(self, x: torch.Tensor, c0, Cn, key):
        y = self.buf(key, (x.shape[0], Cn), torch.float32)
        self._raw(self.lib.stzs_mean_rows, "mean_rows", x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1],
                  x.shape[2], x.shape[1] * x.shape[2], c0, Cn, Cn)
        return y

    # ------------------------------------------------------------------ front ends
    def text_lens(self, text_lens, B: int, T: int):
        """the per-row text lengths of a ragged batch as an int32 [B] device tensor (None stays None): host lengths
        are range-checked (check_text_lens) and uploaded, a device tensor is taken as it is -- no sync, so a front
        given one stays capturable; the kernels clamp what they read into [1, T]."""
        if text_lens is None:
            return None
        if isinstance(text_lens, torch.Tensor) and text_lens.device.type != "cpu":
            if text_lens.dtype != torch.int32 or tuple(text_lens.shape) != (B,) or not text_lens.is_contiguous():
                raise ValueError(f"device text_lens must be a contiguous int32 [{B}] tensor")
            return text_lens
        host = check_text_lens(text_lens, B, T)
        dev = self.buf("text_lens", (B,), torch.int32)
        dev.copy_(host)
        return dev

    def text_encode(self, tokens: torch.Tensor, text_lens=None) -> Act:
        """tokens int32 [B, T] (device) -> h_txt bf16 [B, T, d_txt] (StyleTTS2 TextEncoder):
        embedding gather, te_layers x (k5 conv on MFMA, LayerNorm + LeakyReLU 0.2), then the BiLSTM
        (input projection on MFMA + the register-resident exchange recurrence of csrc/lstm.hip).
        text_lens (DESIGN.md "Ragged text batches"): row b is computed as alone at T = text_lens[b]; the embedding
        and every LayerNorm store its rows t >= text_lens[b] as zeros -- the zero padding the k5 convs see at a
        sequence end -- and the BiLSTM resets its state there, so h_txt[b, text_lens[b]:] = 0."""
        S, W = self.spec, self.W
        B, T = tokens.shape
        lens = self.text_lens(text_lens, B, T)
        e = self.act("te.e", B, T, S.d_txt, self.adt)
        c = self.act("te.c", B, T, S.d_txt, self.adt)
        if lens is not None:
            self._raw(self.lib.stzs_embed_lens, "embed", tokens.data_ptr(), W.t(W.te_emb).data_ptr(), e.ptr,
                      lens.data_ptr(), B, T, S.d_txt, e.ld, e.dt)
        else:
            emb = self.lib.stzs_embed_f32 if self.adt == torch.float32 else self.lib.stzs_embed
            self._raw(emb, "embed", tokens.data_ptr(), W.t(W.te_emb).data_ptr(), e.ptr, B, T, S.d_txt, e.ld)
        for i in range(S.te_layers):
            self.conv(W.te_conv[i], e, c, pad=S.te_kernel // 2, splitk=0 if self.adt == torch.float32 else self.te_splitk,
                      what=f"te.conv{i}")
            g, b = W.te_ln[i]
            self.rowln(c, e, G=W.t(g).data_ptr(), gs=0, Bt=W.t(b).data_ptr(), bs=0, gadd=0.0,
                       act=L.ACT_LEAKY, slope=0.2, lens=lens, what=f"te.ln{i}")
        h = self.act("te.h", B, T, S.d_txt, self.adt)
        return self.lstm(W.te_lstm, e, h, "te.lstm", lens=lens)

    def ref_lens(self, ref_lens, B: int, N: int):
        """the per-row sample counts of a ragged reference batch as an int32 [B] device tensor (None stays None):
        host lengths are range-checked (check_ref_lens) and uploaded, a device tensor is taken as it is -- no sync,
        so a front given one stays capturable; the kernels clamp what they read into [mel_nfft / 2 + 1, N]."""
        if ref_lens is None:
            return None
        if isinstance(ref_lens, torch.Tensor) and ref_lens.device.type != "cpu":
            if ref_lens.dtype != torch.int32 or tuple(ref_lens.shape) != (B,) or not ref_lens.is_contiguous():
                raise ValueError(f"device ref_lens must be a contiguous int32 [{B}] tensor")
            return ref_lens
        host = check_ref_lens(ref_lens, B, N, self.spec.mel_nfft)
        dev = self.buf("ref_lens", (B,), torch.int32)
        dev.copy_(host)
        return dev

    def log_mel(self, wav: torch.Tensor, dtype=None, ref_lens=None) -> Act:
        """reference wav fp32 [B, N] (device) -> log-mel [B, N/hop + 1, n_mels]:
        windowed reflect-padded frames -> bf16 DFT GEMM on MFMA (cos | -sin basis, fp32 out) -> power, sparse
        mel filterbank, log (csrc/frontend.hip); precise_frontend: one stzs_stft_logmel launch (csrc/stftmel.hip).
        dtype of the rows: bf16 | fp32, default the front end's own (fp32 when precise_frontend).
        ref_lens: row b is computed as alone on wav[b, :ref_lens[b]] -- its own reflection, its own
        F_b = ref_lens[b] // hop + 1 frames -- rows t >= F_b of the log-mel are zeros and samples past the length are
        never read.  The STFT launch leaves the F_b in the cached int32 buffer "fe.f_lens" (no host arithmetic)."""
        S, W = self.spec, self.W
        B, N = wav.shape
        Fr = N // S.hop + 1
        if dtype is None:
            dtype = torch.float32 if self.precise_frontend else torch.bfloat16
        lens = self.ref_lens(ref_lens, B, N)
        flens = self.buf("fe.f_lens", (B,), torch.int32) if lens is not None else None
        if self.precise_frontend:
            # one launch, everything in fp32: the frame, an FFT in LDS, power, mel, log (csrc/stftmel.hip)
            mel = self.act("fe.mel", B, Fr, S.n_mels, dtype)
            a = L.StftMelArgs()
            a.wav, a.window, a.twiddle = wav.data_ptr(), W.t(W.fe_win).data_ptr(), W.t(W.fe_tw).data_ptr()
            a.fb, a.ranges, a.y = W.t(W.fe_fb).data_ptr(), W.t(W.fe_rng).data_ptr(), mel.ptr
            a.ldw, a.ldy, a.bsy = N, mel.ld, mel.bs
            a.B, a.N, a.F, a.n_fft, a.win, a.hop = B, N, Fr, S.mel_nfft, S.mel_win, S.hop
            a.n_mels, a.out_dtype = S.n_mels, mel.dt
            if lens is not None:
                a.n_lens, a.f_lens_out = lens.data_ptr(), flens.data_ptr()
            self._call(self.lib.stzs_stft_logmel, a, "stft_logmel")
            return mel
        dft = W.fe_dft
        frames = self.act("fe.frames", B, Fr, dft.ci_pad)
        a = L.FramesArgs()
        a.wav, a.window, a.y = wav.data_ptr(), W.t(W.fe_win).data_ptr(), frames.ptr
        a.ldw, a.ldy, a.bsy = N, frames.ld, frames.bs
        a.B, a.N, a.F, a.n_fft, a.win, a.hop = B, N, Fr, S.mel_nfft, S.mel_win, S.hop
        if lens is not None:
            a.n_lens, a.f_lens_out = lens.data_ptr(), flens.data_ptr()
        self._call(self.lib.stzs_stft_frames, a, "stft_frames")
        nbin = S.mel_nfft // 2 + 1
        spec = self.act("fe.spec", B, Fr, 2 * nbin, torch.float32)
        self.conv(dft, Act(frames.t, 0, S.mel_win), spec, what="fe.dft")
        mel = self.act("fe.mel", B, Fr, S.n_mels, dtype)
        a = L.LogMelArgs()
        a.spec, a.fb, a.ranges, a.y = spec.ptr, W.t(W.fe_fb).data_ptr(), W.t(W.fe_rng).data_ptr(), mel.ptr
        a.lds, a.bss, a.ldy, a.bsy = spec.ld, spec.bs, mel.ld, mel.bs
        a.B, a.F, a.nbin, a.n_mels, a.out_dtype = B, Fr, nbin, S.n_mels, mel.dt
        # (the zero tail frames leave zero spec rows, whose log-mel would be log(1e-5), not the convs' zero padding)
        a.lens = flens.data_ptr() if flens is not None else None
        self._call(self.lib.stzs_log_mel, a, "log_mel")
        return mel

    def prompt_encode(self, ref_wav: torch.Tensor, prompt_idx: torch.Tensor = None, ref_lens=None) -> torch.Tensor:
        """reference-prompt front end on HIP: ref wav [B, N] -> DISCRETE style codes
        (README.md:5): log-mel -> 2 x (k5 conv + LeakyReLU 0.2) -> adaptive average pool to L_s rows ->
        projection -> product VQ (stzs_code_quantize).  Returns the dequantised codes fp32 [B, L_s, code];
        the indices stay in self.prompt_idx [B, L_s, G] (int32).  prompt_idx: teacher-forced indices (the
        front end is skipped, the codebook rows are gathered; ref_lens is then ignored, as ref_wav is).
        ref_lens: per-row sample counts of a ragged reference batch (prompt_features)."""
        S, W = self.spec, self.W
        G = S.code_dim // S.vq_group
        if prompt_idx is not None:
            B = prompt_idx.shape[0]
            idx = self.buf("prompt.idx", (B, S.L_s, G), torch.int32)
            idx.copy_(prompt_idx.to(torch.int32).reshape(B, S.L_s, G))
            out = self.buf("prompt", (B, S.L_s, S.code_dim), torch.float32)
            self.code_quantize(None, idx, out, lookup=True)
            self.prompt_idx = idx
            return out
        z = self.prompt_features(ref_wav, ref_lens)
        B = z.shape[0]
        idx = self.buf("prompt.idx", (B, S.L_s, G), torch.int32)
        out = self.buf("prompt", (B, S.L_s, S.code_dim), torch.float32)
        self.code_quantize(z, idx, out)
        self.prompt_idx = idx
        return out

    def code_quantize(self, z, idx: torch.Tensor, out: torch.Tensor, lookup=False):
        """product VQ of z fp32 [B, L, code] -> idx int32 [B, L, G] + dequantised rows out (lookup: idx given)."""
        S, W = self.spec, self.W
        a = L.VqArgs()
        a.x = z.data_ptr() if z is not None else None
        a.codebook, a.idx, a.y = W.t(W.pe_vq).data_ptr(), idx.data_ptr(), out.data_ptr()
        G = S.code_dim // S.vq_group
        a.ldx, a.ldi, a.ldy = S.code_dim, G, S.code_dim
        a.R, a.G, a.K, a.dg, a.lookup = idx.shape[0] * idx.shape[1], G, S.vq_size, S.vq_group, int(lookup)
        self._call(self.lib.stzs_code_quantize, a, "code_quantize")

    def prompt_features(self, ref_wav: torch.Tensor, ref_lens=None) -> torch.Tensor:
        """ref wav [B, N] -> continuous prompt codes fp32 [B, L_s, code] (before the quantiser).
        ref_lens: int [B] (host: range-checked; int32 device tensor: trusted, no sync), each in
        [mel_nfft / 2 + 1, N] -- a ragged reference batch: row b is computed as alone on ref_wav[b, :ref_lens[b]]
        (what lies past it is never read).  The log-mel carries the lengths (log_mel); the convs run over the padded
        block and need none: zero log-mel tail rows are the zero padding pe.conv0 sees at a clip's end, one
        stzs_mask_rows launch makes the tail rows of its output (LeakyReLU(bias)) that padding for pe.conv1, what
        pe.conv1 leaves in its own tail rows is never read, and the pool averages each row over its own frames."""
        S, W = self.spec, self.W
        wav = ref_wav.to(self.device, torch.float32).contiguous()
        B = wav.shape[0]
        lens = self.ref_lens(ref_lens, B, wav.shape[1])
        mel = self.log_mel(wav, ref_lens=lens)
        flens = self.buf("fe.f_lens", (B,), torch.int32) if lens is not None else None  # (written by the STFT launch)
        Fr = mel.T
        # (precise_frontend: fp32 rows; the convs then take the split-operand route on the weights' hi | lo streams)
        fdt = torch.float32 if self.precise_frontend else torch.bfloat16
        c0 = self.act("fe.c0", B, Fr, S.pe_ch, fdt)
        c1 = self.act("fe.c1", B, Fr, S.pe_ch, fdt)
        self.conv(W.pe_conv0, mel, c0, pad=2, epi_act=L.ACT_LEAKY, epi_slope=0.2, what="pe.conv0")
        if flens is not None:
            a = L.MaskArgs()
            a.x, a.lens, a.ld, a.bs = c0.ptr, flens.data_ptr(), c0.ld, c0.bs
            a.B, a.T, a.C, a.dtype = B, Fr, S.pe_ch, c0.dt
            self._call(self.lib.stzs_mask_rows, a, "mask_rows")
        self.conv(W.pe_conv1, c0, c1, pad=2, epi_act=L.ACT_LEAKY, epi_slope=0.2, what="pe.conv1")
        pooled = self.act("fe.pool", B, S.L_s, S.pe_ch, fdt)
        a = L.PoolArgs()
        a.x, a.y, a.ldx, a.bsx, a.ldy, a.bsy = c1.ptr, pooled.ptr, c1.ld, c1.bs, pooled.ld, pooled.bs
        a.B, a.T, a.L, a.C, a.in_dtype, a.out_dtype = B, Fr, S.L_s, S.pe_ch, c1.dt, pooled.dt
        a.lens = flens.data_ptr() if flens is not None else None
        self._call(self.lib.stzs_pool_rows, a, "pool_rows")
        out = self.buf("prompt.z", (B, S.L_s, S.code_dim), torch.float32)
        self.conv(W.pe_proj, pooled, Act(out), what="pe.proj")
        return out

    # ------------------------------------------------------------------ enrolled voices
    def voice_prompt(self, zbank: torch.Tensor, ibank, src: torch.Tensor, w: torch.Tensor, cnt: torch.Tensor,
                     idx: torch.Tensor, out: torch.Tensor, zmix: torch.Tensor = None, gather=False):
        """one stzs_voice_prompt launch: zbank fp32 [V, L, code] (ibank int32 [V, L, G]: the gather form's input), src
        int32 [B, Kmax], w fp32 [B, Kmax], cnt int32 [B] on the device -> idx int32 [B, L, G], out fp32 [B, L, code]
        (the dequantised rows), zmix fp32 [B, L, code] (optional: the mixed pre-quantiser rows)"""
        S, W = self.spec, self.W
        G = S.code_dim // S.vq_group
        a = L.VoiceArgs()
        a.zbank, a.ibank = zbank.data_ptr(), (ibank.data_ptr() if ibank is not None else None)
        a.codebook, a.src, a.w, a.cnt = W.t(W.pe_vq).data_ptr(), src.data_ptr(), w.data_ptr(), cnt.data_ptr()
        a.idx, a.y, a.zmix = idx.data_ptr(), out.data_ptr(), (zmix.data_ptr() if zmix is not None else None)
        a.ldz, a.ldib, a.ldi, a.ldy, a.ldm = S.code_dim, G, G, S.code_dim, S.code_dim
        a.V, a.L, a.B, a.Kmax = zbank.shape[0], zbank.shape[1], idx.shape[0], src.shape[1]
        a.G, a.K, a.dg, a.gather = G, S.vq_size, S.vq_group, int(bool(gather))
        self._call(self.lib.stzs_voice_prompt, a, "voice_prompt")

    def voice_encode(self, voices: "VC.VoiceRows") -> torch.Tensor:
        """the prompt of a batch from enrolled voices, ONE launch: -> the dequantised codes fp32 [B, L_s, code], what
        prompt_encode returns; the indices stay in self.prompt_idx.  The kernel reads the rows' device arrays (and the
        bank's) when it runs: a captured graph replays with what VoiceRows.set() / VoiceBank.replace() wrote."""
        S = self.spec
        B = voices.B
        G = S.code_dim // S.vq_group
        bank = voices.bank
        if tuple(bank.z.shape[1:]) != (S.L_s, S.code_dim) or bank.z.device != self.device or \
                voices.src.device != self.device or (bank.idx is None and voices.gather) or \
                (bank.idx is not None and tuple(bank.idx.shape) != (bank.z.shape[0], S.L_s, G)):
            raise ValueError("voices: the bank or the rows do not belong to this engine (shape / device)")
        idx = self.buf("prompt.idx", (B, S.L_s, G), torch.int32)
        out = self.buf("prompt", (B, S.L_s, S.code_dim), torch.float32)
        self.voice_prompt(bank.z, bank.idx, voices.src, voices.w, voices.cnt, idx, out, gather=voices.gather)
        self.prompt_idx = idx
        return out

    def voice_fingerprint(self) -> str:
        """what a Voice must carry to be used with this engine (stzs/voice.py engine_fingerprint)"""
        return VC.engine_fingerprint(self)

    def enroll(self, ref_wav, ref_lens=None, ref_sr=None, weights=None) -> "VC.Voice":
        """enrol a voice: ref_wav fp32 [N], or [K, N] -- K <= 8 clips of one speaker, zero-padded and
        ragged through ref_lens, at any rate through ref_sr (both as synth() takes them) -> Voice.  The K clips run as
        ONE prompt_features batch; one stzs_voice_prompt launch in the mix form then forms
        z = sum_k w_k z_k, w_k = float32(weights_k / sum(weights)) (float64 on the host; default: equal), and its
        discrete codes.  With one clip the weight is exactly 1.0 and the voice holds, bit for bit, what
        prompt_features / prompt_encode give for the clip.  ValueError -- before any launch -- for K > 8, a
        non-finite or negative weight, a zero sum."""
        S = self.spec
        wav = torch.as_tensor(ref_wav)
        if wav.dim() == 1:
            wav = wav[None]
        if wav.dim() != 2 or not wav.dtype.is_floating_point:
            raise ValueError(f"enroll: ref_wav must be a float [N] or [K, N] tensor, got {tuple(wav.shape)} {wav.dtype}")
        K = wav.shape[0]
        if not 1 <= K <= VC.KMAX:
            raise ValueError(f"enroll: {K} clips (1 to {VC.KMAX} per voice)")
        w = VC.normalise_weights(weights, K, "enroll: weights")
        if ref_sr is not None:
            wav, ref_lens = self._ref_in(wav, ref_sr, ref_lens, None)
        z = self.prompt_features(wav, ref_lens)
        G = S.code_dim // S.vq_group
        dev = self.device
        src = torch.arange(K, dtype=torch.int32).reshape(1, K).to(dev)
        wd = torch.tensor([w], dtype=torch.float32).to(dev)
        cnt = torch.tensor([K], dtype=torch.int32).to(dev)
        idx = torch.empty(1, S.L_s, G, dtype=torch.int32, device=dev)
        q = torch.empty(1, S.L_s, S.code_dim, dtype=torch.float32, device=dev)
        zmix = torch.empty(1, S.L_s, S.code_dim, dtype=torch.float32, device=dev)
        self.voice_prompt(z, None, src, wd, cnt, idx, q, zmix)
        return VC.Voice(zmix[0], idx[0], self.voice_fingerprint(), K, "precise" if self.precise_frontend else "bf16")

    def voice_rows(self, B: int, bank, ids, weights=None) -> "VC.VoiceRows":
        """the speakers of a batch of B rows (VoiceRows): ids is B voice ids of `bank` (one voice per
        row: the gather form), or B id sequences with B weight sequences (blends, rows of different source counts: the
        mix form; weights None: equal).  Host values are range-checked (ValueError) and uploaded once into device
        arrays the result owns; hand it to synth / synth_stream / encode_inputs as voices=."""
        return VC.VoiceRows(B, bank, ids, weights, self.device)

    def _check_voices(self, voices, tokens, ref_wav=None, prompt_idx=None, ref_lens=None, ref_sr=None):
        """voices= excludes every other source of the prompt, and is made for the batch's row count: ValueError,
        before any launch"""
        if voices is None:
            return
        for name, v in (("ref_wav", ref_wav), ("prompt_idx", prompt_idx), ("ref_lens", ref_lens), ("ref_sr", ref_sr)):
            if v is not None:
                raise ValueError(f"voices= and {name}= were both given: the prompt comes from one or the other")
        if not isinstance(voices, VC.VoiceRows):
            raise ValueError(f"voices must be VoiceRows (voice_rows()), got {type(voices).__name__}")
        voices.rows(tokens.shape[0])

    # ------------------------------------------------------------------ (a) style diffusion
    def sample_style(self, h_txt: Act, prompt: torch.Tensor, eps: torch.Tensor, steps: int,
                     cfg_scale: float = 1.0, text_lens=None, controls: RowControls = None) -> torch.Tensor:
        """a1-a4: Euler sampling over the distilled / Karras sigma schedule with classifier-free guidance.
        h_txt [B, T, d_txt] bf16, prompt [B, L_s, code] fp32, eps [B, L_s, code] -> codes fp32 [B, L_s, code].
        text_lens: row b's cross-attention sees its first text_lens[b] text rows, then the prompt (denoiser_prepare).
        controls: a cfg_scale of theirs replaces the argument -- a scalar as the argument would, B values as one
        guidance scale per row (the CFG form when any differs from 1: stzs_cfg_euler_rows; a row at exactly 1 takes
        its conditional prediction alone)."""
        S = self.spec
        B = h_txt.B
        scales = None
        if controls is not None:
            controls.rows(B)
            if controls.cfg is not None:
                cfg_scale = 1.0
                scales = controls.cfg if controls.cfg_form else None
            elif controls.cfg_scalar is not None:
                cfg_scale = controls.cfg_scalar
        cfg = cfg_scale != 1.0 or scales is not None
        R = 2 * B if cfg else B
        sig = sigma_schedule(S, steps)
        if h_txt.t.dtype != self.sdt:  # (the long-form mode: precise fp32 text rows into the bf16 / fp8 sampler)
            hs = self.act("dn.h_txt", B, h_txt.T, h_txt.C, self.sdt)
            self.copy2d(h_txt, hs, h_txt.T, h_txt.C)
            h_txt = hs
        st = self.denoiser_prepare(h_txt, prompt, sig[:steps], cfg, text_lens)
        x = self.buf("dn.x", (R, S.L_s, S.code_dim), torch.float32)
        N = S.L_s * S.code_dim
        self._raw(self.lib.stzs_state_init, "state_init", x.data_ptr(), eps.data_ptr(), B, N, int(cfg), float(sig[0]))
        D = self.act("dn.D", R, S.L_s, S.code_dim, torch.float32)
        for i in range(steps):
            self.denoiser_step(st, i, Act(x), D)
            if scales is not None:
                self._raw(self.lib.stzs_cfg_euler_rows, "cfg_euler_rows", x.data_ptr(), D.t.data_ptr(), B, N,
                          scales.data_ptr(), float(sig[i]), float(sig[i + 1] - sig[i]))
                continue
            self._raw(self.lib.stzs_cfg_euler, "cfg_euler", x.data_ptr(), D.t.data_ptr(), B, N, int(cfg),
                      float(cfg_scale), float(sig[i]), float(sig[i + 1] - sig[i]))
        return x[:B]

    def denoiser_fwd(self, h_txt: Act, prompt: torch.Tensor, x: torch.Tensor, sigma: float, cfg: bool) -> torch.Tensor:
        """a2 alone: ONE preconditioned denoiser evaluation D(x, sigma) (EDM c_skip / c_out / c_in / c_noise) on the
        rows x [R, L_s, code] fp32 (R = 2B with CFG: conditional rows, then the null-prompt rows) -> D fp32
        [R, L_s, code] (a device buffer of the engine)."""
        S = self.spec
        st = self.denoiser_prepare(h_txt, prompt, [float(sigma)], cfg)
        D = self.act("dn.D", x.shape[0], S.L_s, S.code_dim, torch.float32)
        self.denoiser_step(st, 0, Act(x), D)
        return D.t

    def denoiser_prepare(self, h_txt: Act, prompt: torch.Tensor, sigmas, cfg: bool, text_lens=None) -> dict:
        """step-invariant part of a sampling run: the cross-attention context [ctx_txt(h) ; ctx_prm(prompt | null)]
        and its per-layer K/V, the pooled prompt, and the conditioning of EVERY sigma at once (rows s * R + r):
        adaLN-single input, its two projections and the per-layer expansion -> 5 launches instead of 5 per NFE.
        text_lens (ragged batch): the text context is written over all T rows, row r's prompt (null) context is
        packed behind its own text rows -- ctx[r, len_r : len_r + L_s] -- and its cross-attention reads
        lk_rows[r] = len_r + L_s keys: the keys of that row alone, in the same order.  Context / K / V rows past
        them are computed and never read."""
        S, W = self.spec, self.W
        B, T = h_txt.B, h_txt.T
        R = 2 * B if cfg else B
        Ls, d, cd = S.L_s, S.dn_d, S.code_dim
        Lc = T + Ls
        steps = len(sigmas)
        lens = self.text_lens(text_lens, B, T)
        lk = None
        ctx = self.act("dn.ctx", R, Lc, d, self.sdt)
        # ctx_txt rows: the conv writes T rows per utterance into a buffer of Lc rows per utterance
        self._conv_rows(W.dn_ctx_txt, h_txt, ctx.t, 0, 0, "dn.ctx_txt")
        pa = Act(prompt)
        esz = ctx.t.element_size()
        if lens is None:
            self._conv_rows(W.dn_ctx_prm, pa, ctx.t, 0, T, "dn.ctx_prm")
        else:  # the prompt context beside the buffer, then each row's copy to behind its own text rows
            cp = self.act("dn.ctx_prm", B, Ls, d, self.sdt)
            self.conv(W.dn_ctx_prm, pa, cp, what="dn.ctx_prm")
            # the copies' destination row offsets: the lengths clamped into [1, T] on the device (a device
            # text_lens is not checked on the host: whatever it holds, the copies stay inside ctx), and the key
            # counts from them -- stream-ordered device ops into cached buffers, capturable
            lens = torch.clamp(lens, 1, T, out=self.buf("dn.row_off", (B,), torch.int32))
            lk = self.buf("dn.lk_rows", (R,), torch.int32)
            for r0 in range(0, R, B):
                torch.add(lens, Ls, out=lk[r0:r0 + B])
            self._copy_rows(cp.ptr, cp.ld, cp.bs, ctx.ptr, ctx.ld, ctx.bs, B, Ls, d, cp.dt, ctx.dt, "ctx_prm_pack",
                            row_off=lens)
        if cfg:
            self._conv_rows(W.dn_ctx_txt, h_txt, ctx.t, B, 0, "dn.ctx_txt.u")
            f32 = self.sdt == torch.float32
            nul = Act(W.t(W.dn_ctx_null32 if f32 else W.dn_ctx_null)[None])
            dst = Act(ctx.t[B:]).rows(0, B)
            if lens is None:
                self._copy_rows(nul.ptr, d, 0, dst.t.data_ptr() + T * ctx.ld * esz, ctx.ld, Lc * ctx.ld,
                                B, Ls, d, nul.dt, ctx.dt, "ctx_null")
            else:
                self._copy_rows(nul.ptr, d, 0, dst.t.data_ptr(), ctx.ld, Lc * ctx.ld, B, Ls, d, nul.dt, ctx.dt,
                                "ctx_null", row_off=lens)
        pm = self.mean_rows(prompt, 0, cd, "dn.pm")
        pool = self.buf("dn.pool", (R, d), torch.float32)
        self.conv(W.dn_pool, Act(pm[:, None]), Act(pool[:B, None]), rows=self._rows_z(W.dn_pool), what="dn.pool")
        if cfg:
            self._copy_rows(W.t(W.dn_pool_null).data_ptr(), d, 0, pool[B:].data_ptr(), d, d, B, 1, d, L.F32, L.F32,
                            "pool_null")
        kv = []
        if getattr(W, "dn_kv_all", None) is not None and self.kv_fuse:
            # (r06) all layers' K / V of the shared context in one linear (weights.py dn_kv_all); layer l's [K | V] are
            # channels [2 d l, 2 d (l + 1)) of its rows
            nl = len(W.dn_layers)
            kva = self.act("dn.kv_all", R, Lc, 2 * d * nl, self.sdt)
            self.conv(W.dn_kv_all, ctx, kva, what="dn.kv")
            kv = [Act(kva.t, 2 * d * l, 2 * d) for l in range(nl)]
        else:
            for l, lw in enumerate(W.dn_layers):
                kvl = self.act(f"dn.kv{l}", R, Lc, 2 * d, self.sdt)
                self.conv(lw["kv"], ctx, kvl, what=f"dn.kv{l}")
                kv.append(kvl)
        # sigma embeddings for all steps
        fkey = ("dn.four", tuple(float(v) for v in sigmas))
        fo = self._consts.get(fkey)
        if fo is None:  # host constant, uploaded once (never inside a graph capture)
            four = np.stack([fourier_features(S, edm_coeffs(S, v)["c_noise"]) for v in sigmas])
            fo = self._consts[fkey] = torch.from_numpy(four)[None].to(self.device)
        t0 = self.act("dn.t0", 1, steps, d, torch.float32)
        temb = self.act("dn.temb", 1, steps, d, torch.float32)
        self.conv(W.dn_t0, Act(fo), t0, epi_act=L.ACT_SILU, rows=self._rows_z(W.dn_t0), what="dn.t0")
        self.conv(W.dn_t1, t0, temb, rows=self._rows_z(W.dn_t1), what="dn.t1")
        cb = self.buf("dn.cb", (steps * R, d), self.sdt)
        mod = self.buf("dn.mod", (steps * R, 6 * d), torch.float32)
        fmod = self.buf("dn.fmod", (steps * R, 2 * d), torch.float32)
        modx = self.buf("dn.modx", (S.dn_layers, steps * R, 6 * d), torch.float32)
        fmodx = self.buf("dn.fmodx", (1, steps * R, 2 * d), torch.float32)
        cond = self.lib.stzs_dn_cond_steps_f32 if cb.dtype == torch.float32 else self.lib.stzs_dn_cond_steps
        self._raw(cond, "dn_cond_steps", pool.data_ptr(), temb.t.data_ptr(), cb.data_ptr(), R, d, steps)
        self.conv(W.dn_ada, Act(cb[:, None]), Act(mod[:, None]), what="dn.ada")
        self.conv(W.dn_final_ada, Act(cb[:, None]), Act(fmod[:, None]), what="dn.final_ada")
        self._raw(self.lib.stzs_adaln_expand, "adaln_expand", mod.data_ptr(), W.t(W.dn_table).data_ptr(),
                  modx.data_ptr(), steps * R, d, 6, S.dn_layers, 0b010010)
        self._raw(self.lib.stzs_adaln_expand, "adaln_expand.f", fmod.data_ptr(), None, fmodx.data_ptr(), steps * R, d,
                  2, 1, 0b10)
        return dict(R=R, sig=list(sigmas), kv=kv, modx=modx, fmodx=fmodx, lk=lk)

    def denoiser_step(self, st: dict, i: int, xa: Act, D: Act):
        """one NFE: D = c_skip x + c_out F(c_in x, sigma_i) for the R rows of xa, with the conditioning prepared
        by denoiser_prepare (6 layers: adaLN-modulated self-attention, cross-attention, GELU FFN)."""
        S, W = self.spec, self.W
        R, kv, modx, fmodx = st["R"], st["kv"], st["modx"], st["fmodx"]
        Ls, d = S.L_s, S.dn_d
        h = self.act("dn.h", R, Ls, d, torch.float32)
        an = self.act("dn.a", R, Ls, d, self.sdt)
        qkv = self.act("dn.qkv", R, Ls, 3 * d, self.sdt)
        o = self.act("dn.o", R, Ls, d, self.sdt)
        q = self.act("dn.q", R, Ls, d, self.sdt)
        ff = self.act("dn.ff", R, Ls, S.dn_ffn, self.sdt)
        pos = Act(W.t(W.dn_pos)[None])
        fsz = 4
        f8 = self.fp8_denoiser
        if f8:  # e4m3fn operand rows + per-row scales for the layer linears
            an8 = self.act("dn.a8", R, Ls, d, torch.float8_e4m3fn)
            o8 = self.act("dn.o8", R, Ls, d, torch.float8_e4m3fn)
            ff8 = self.act("dn.ff8", R, Ls, S.dn_ffn, torch.float8_e4m3fn)
            s_an = self.buf("dn.a8s", (R * Ls,), torch.float32)
            s_o = self.buf("dn.o8s", (R * Ls,), torch.float32)
            s_ff = self.buf("dn.ff8s", (R * Ls,), torch.float32)
        co = edm_coeffs(S, st["sig"][i])
        rk = {} if (f8 or self.sdt == torch.float32) else self.dn_rows
        if f8:
            ain, sin, sfx = an8, s_an, "8"
        else:
            ain, sin, sfx = an, None, ""
        # adaLN / LayerNorm rows of this step: ln1_l, ca_ln_l, ln2_l for every layer, then lnf; each one
        # after the first is launched right behind the residual linear that produces its input (post_ln), or on the
        # rows form runs inside the linear that reads it (pre_ln, stzs_ln_linear).
        # (Fusing them into that linear's epilogue -- last-arriving tile of a row block, sc1 hand-off --
        # was tried: bit-identical but 1.6x slower at batch 1, the block's rows then normalise on one CU.)
        lns = []
        for l, lw in enumerate(W.dn_layers):
            mb = modx[l, i * R].data_ptr()  # this step's rows of layer l's modulation
            lns.append(self._ln_args(h, ain, G=mb + d * fsz, gs=6 * d, Bt=mb, bs=6 * d, gdiv=Ls, y_scale=sin))
            lns.append(self._ln_args(h, ain, G=W.t(lw["ln_g"]).data_ptr(), Bt=W.t(lw["ln_b"]).data_ptr(),
                                     y_scale=sin))
            lns.append(self._ln_args(h, ain, G=mb + 4 * d * fsz, gs=6 * d, Bt=mb + 3 * d * fsz, bs=6 * d, gdiv=Ls,
                                     y_scale=sin))
        fb = fmodx[0, i * R].data_ptr()
        lns.append(self._ln_args(h, an, G=fb + d * fsz, gs=2 * d, Bt=fb, bs=2 * d, gdiv=Ls))
        # on the rows form each LayerNorm runs inside the linear that reads it (pre_ln) instead of behind its producer
        fl = bool(rk) and self.ln_fuse
        post = lambda k: None if fl else lns[k]
        pre = lambda k: lns[k] if fl else None
        self.conv(W.dn_in, xa, h, cscale=co["c_in"], res=pos, rows=rk.get("inp", 0), post_ln=post(0), what="dn.in")
        sk = {} if (f8 or self.sdt == torch.float32) else self.dn_splitk
        for l, lw in enumerate(W.dn_layers):
            mb = modx[l, i * R].data_ptr()
            self.conv(lw["qkv" + sfx], ain, qkv, x_scale=sin, splitk=sk.get("qkv", 0), rows=rk.get("qkv", 0),
                      pre_ln=pre(3 * l), attn=(qkv.sl(0, d), qkv.sl(d, d), qkv.sl(2 * d, d), o), what="qkv")
            xo, so = (o8, s_o) if f8 else (o, None)
            if f8:
                self.quant(o, o8, s_o)
            self.conv(lw["o" + sfx], xo, h, res=h, gate=mb + 2 * d * fsz, gate_bs=6 * d, x_scale=so,
                      post_ln=post(3 * l + 1), splitk=sk.get("o", 0), rows=rk.get("o", 0), what="sa_o")
            self.conv(lw["q" + sfx], ain, q, x_scale=sin, splitk=sk.get("q", 0), rows=rk.get("q", 0),
                      pre_ln=pre(3 * l + 1), attn=(q, kv[l].sl(0, d), kv[l].sl(d, d), o, st.get("lk")), what="ca_q")
            if f8:
                self.quant(o, o8, s_o)
            self.conv(lw["co" + sfx], xo, h, res=h, x_scale=so, post_ln=post(3 * l + 2), splitk=sk.get("co", 0),
                      rows=rk.get("co", 0), what="ca_o")
            self.conv(lw["ff1" + sfx], ain, ff, epi_act=L.ACT_GELU, x_scale=sin, splitk=sk.get("ff1", 0),
                      rows=rk.get("ff1", 0), pre_ln=pre(3 * l + 2), what="ff1")
            xf, sf = (ff8, s_ff) if f8 else (ff, None)
            if f8:
                self.quant(ff, ff8, s_ff)
            self.conv(lw["ff2" + sfx], xf, h, res=h, gate=mb + 5 * d * fsz, gate_bs=6 * d, x_scale=sf,
                      post_ln=post(3 * l + 3), splitk=sk.get("ff2", 0), rows=rk.get("ff2", 0), what="ff2")
        self.conv(W.dn_out, an, D, alpha=co["c_out"], acc_in=xa, beta=co["c_skip"], rows=rk.get("out", 0),
                  pre_ln=pre(len(lns) - 1), what="dn.out")

    def _ln_args(self, x: Act, y: Act, *, G=None, gs=0, Bt=None, bs=0, gdiv=1, gadd=0.0, y_scale=None):
        """stzs_rowln_args of a modulated LayerNorm x -> y (launched by stzs_row_layernorm behind the linear that
        produces x: conv(post_ln=...))."""
        a = L.RowLNArgs()
        a.x, a.y, a.G, a.Bt = x.ptr, y.ptr, G, Bt
        a.ldx, a.ldy, a.gs, a.bs = x.ld, y.ld, gs, bs
        a.R, a.C, a.gdiv, a.in_dtype, a.out_dtype, a.act = x.B * x.T, x.C, gdiv, x.dt, y.dt, L.ACT_NONE
        a.gadd, a.eps, a.slope = gadd, 1e-5, 0.0
        a.y_scale = y_scale.data_ptr() if y_scale is not None else None
        return a

    def _conv_rows(self, cw, x: Act, dst: torch.Tensor, b0, t0, what):
        """linear over x [B, T, C] written to dst[b0 + b, t0 + t, :] (dst rows have a larger T)."""
        B, T = x.B, x.T
        y = Act(dst[b0:b0 + B])
        a_y = Act(y.t, 0, cw.Co)
        # shift the output base by t0 rows; the batch stride stays that of dst
        view = _OffsetAct(a_y, t0 * dst.shape[2])
        self.conv(cw, x, view, T_out=T, what=what)

    # ------------------------------------------------------------------ (b) prosody predictor
    def predict_prosody(self, h_txt: Act, codes: torch.Tensor, durations=None, n_frames=None, text_lens=None,
                        ragged_frames=False, controls: RowControls = None):
        """durations: optional int tensor [B, T_txt] (host or device); n_frames: their per-utterance sum if
        known (avoids the device->host sync, e.g. under graph capture).  Returns dict of device tensors.
        text_lens: ragged text rows (duration_encoder); the padding tokens get duration 0 and the alignment never
        references them, so the batch still only has to share its frame count.
        ragged_frames: the rows need not share their frame count: the batch runs at the padded width T40 = the
        longest row's (or n_frames, then the padded width: no host sync at all), each row on its own frames
        (prosody_frames; the result gains "frame_lens").
        controls: their speed divides row b's predicted durations (duration_head; forced durations win), so rows of
        different rates have different frame counts and need ragged_frames; their pitch_shift multiplies F0
        (f0n_predictor)."""
        if ragged_frames:
            self._check_ragged_frames()
        if controls is not None:
            controls.rows(h_txt.B)
        text_lens = self.text_lens(text_lens, h_txt.B, h_txt.T)
        if self.dur_overlap and durations is not None and (n_frames is not None or durations.device.type == "cpu"):
            # the alignment reads the given durations, so the duration LSTM no longer gates the frame branch: it
            # runs in ONE launch with the shared F0/N LSTM (stzs_lstm_pair), its projection and the durations kernel
            # after the F0/N branches -- every output the same bits as the sequential order
            d, ov = self.duration_encoder(h_txt, codes, durations, text_lens)
            if n_frames is not None:
                T40 = int(n_frames)
            else:
                tot = durations.to(torch.int64)
                if text_lens is not None:  # (forced durations of padding tokens do not count: the kernel zeroes them)
                    tot = tot * (torch.arange(h_txt.T)[None] < text_lens.cpu()[:, None])
                tot = tot.sum(1)
                assert ragged_frames or int(tot.min()) == int(tot.max()), \
                    "one batch must share its total frame count (stzs.scheduler.BucketScheduler groups by it)"
                T40 = int(tot.max())
            if text_lens is not None:  # the alignment reads the durations with the padding tokens' zeroed
                ov = self._mask_durations(ov, text_lens)
            pro = self.prosody_frames(h_txt, codes, d, ov, T40, pair_dur=True, text_lens=text_lens,
                                      ragged_frames=ragged_frames, controls=controls)
            du = self.duration_head(d, ov, hd=pro.pop("_hd"), text_lens=text_lens, controls=controls)
            pro.update(du, dur=du["dur"])
            return pro
        du = self.predict_durations(h_txt, codes, durations, text_lens, controls)
        if n_frames is not None:
            T40 = int(n_frames)
        else:
            if durations is not None and durations.device.type == "cpu" and text_lens is None:
                tot = durations.to(torch.int64).sum(1)
            else:
                tot = du["dur"].to(torch.int64).sum(1).cpu()  # host sync: the frame count sizes every later buffer
            assert ragged_frames or int(tot.min()) == int(tot.max()), \
                "one batch must share its total frame count (stzs.scheduler.BucketScheduler groups by it)"
            T40 = int(tot.max())
        return self.prosody_frames(h_txt, codes, du["d"], du["dur"], T40, du, ragged_frames=ragged_frames,
                                   controls=controls)

    def _check_ragged_frames(self):
        """ragged frames run where the block convs take the lengths: the default engine's forms and the precise
        engines' mrfx / conv_x3 forms (every fp32 block conv must carry split-operand weights, which a
        precise engine's packed model does) -- not the latency engine's split-K / pair convs (before any launch)"""
        if self.blk_splitk:
            raise NotImplementedError("ragged_frames: not on a blk_splitk (latency) engine -- its split-K / pair "
                                      "block convs do not take per-row lengths")
        if self.precise or self.precise_all:
            # fp32 blocks (the decoder's; with precise_all the predictor's too): their k3 convs take the lengths on the
            # split-operand forms only -- every one must carry such weights (none packed: nothing to vouch for)
            W = getattr(self, "W", None)
            blks = [] if W is None else \
                [b for b in list(W.dec_blk.values()) + (list(W.pr_blk.values()) if self.precise_all else [])
                 if hasattr(b, "conv1")]
            if not blks or not all(getattr(c, "wx3", None) is not None or getattr(c, "fx3", None) is not None
                                   for b in blks for c in (b.conv1, b.conv2)):
                raise NotImplementedError("ragged_frames: a precise engine's block convs take per-row lengths on the "
                                          "split-operand forms (mrfx, conv_x3) only, not on conv_f32")

    def prosody_rows(self, pro: dict, rows, T_b: int) -> dict:
        """rows (indices) of a ragged-frames result that share the frame count T_b -> a pro dict decode() accepts for
        them: asr_buf[b, :T_b, :d_txt], F0[b, :2 T_b] and N[b, :2 T_b] copied into fresh buffers (data movement only;
        the source may be overwritten by the next prosody batch, and decode() fills the copy's F0 / N columns)."""
        S = self.spec
        T_b = int(T_b)
        assert 1 <= T_b <= pro["T40"], (T_b, pro["T40"])
        ix = torch.as_tensor(list(rows), dtype=torch.int64, device=self.device)
        src = pro["asr_buf"]
        asr = torch.zeros(len(ix), T_b, src.t.shape[2], dtype=src.t.dtype, device=self.device)
        asr[:, :, :S.d_txt] = src.t[ix, :T_b, src.c0:src.c0 + S.d_txt]
        return dict(asr_buf=Act(asr, 0, S.d_txt + 2), F0=pro["F0"][ix, :2 * T_b].contiguous(),
                    N=pro["N"][ix, :2 * T_b].contiguous(), T40=T_b)

    def predict_durations(self, h_txt: Act, codes: torch.Tensor, durations=None, text_lens=None,
                          controls: RowControls = None) -> dict:
        """a5-a6: DurationEncoder + duration LSTM + head -> dict(dur int32 [B, T], dsum, logits, d) (device).
        text_lens (ragged batch): dur[b, :text_lens[b]] and d[b, :text_lens[b]] are those of row b alone at
        T = text_lens[b]; dur is 0 past it (forced or not), d / logits / dsum rows past it are unspecified, finite.
        controls: their speed, as duration_head."""
        text_lens = self.text_lens(text_lens, h_txt.B, h_txt.T)
        d, ov = self.duration_encoder(h_txt, codes, durations, text_lens)
        return self.duration_head(d, ov, text_lens=text_lens, controls=controls)

    def _mask_durations(self, ov: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """given durations with those of the padding tokens (t >= lens[b]) zeroed, in the engine's own buffer
        (device ops, stream-ordered; the caller's tensor is left as it is)"""
        out = self.buf("pr.dur_ovm", tuple(ov.shape), torch.int32)
        keep = torch.arange(ov.shape[1], device=ov.device, dtype=torch.int32)[None] < lens[:, None]
        torch.mul(ov, keep, out=out)
        return out

    def duration_encoder(self, h_txt: Act, codes: torch.Tensor, durations=None, text_lens=None):
        """a5: DurationEncoder (LSTM + AdaLN layers) -> (d [B, T, pr_in], the given durations as an int32 device
        tensor -- the caller's own when it is one (contiguous [B, T]: read in place, stream-ordered), else the copy
        pr.dur_ov -- or None).  text_lens (ragged batch): the style is resampled to each row's own length and the
        BiLSTMs reset at its end; what the AdaLN layers leave in the padding rows is never read by a kept row."""
        S, W = self.spec, self.W
        B, T = h_txt.B, h_txt.T
        lens = self.text_lens(text_lens, B, T)
        pin = S.pr_in
        xin = self.act("pr.xin", B, T, pin, self.adt)
        assert h_txt.t.dtype == self.adt
        a = L.PrPrepArgs()
        a.codes, a.h, a.y = codes.data_ptr(), h_txt.ptr, xin.ptr
        a.ldc, a.bsc, a.ldh, a.bsh, a.ldy, a.bsy = codes.shape[2], codes.shape[1] * codes.shape[2], h_txt.ld, \
            h_txt.bs, xin.ld, xin.bs
        a.B, a.L, a.T, a.c0, a.Cs, a.Ch, a.yc0 = B, S.L_s, T, S.style_ac, S.style_pr, S.d_txt, S.d_txt
        a.f32 = int(self.adt == torch.float32)
        a.lens = lens.data_ptr() if lens is not None else None
        self._call(self.lib.stzs_predictor_prep, a, "pr_prep")
        hout = self.act("pr.hout", B, T, S.pr_hid, self.adt)
        nl = S.pr_layers
        if getattr(W, "pr_aln_all", None) is not None and self.kv_fuse:
            # (r06) every layer's AdaLN gamma / beta from the style columns (never rewritten by the layers: d_txt ==
            # pr_hid) in one stacked linear, layer i's at channels [2 pr_hid i, 2 pr_hid (i + 1))
            gb = self.act("pr.gb_all", B, T, 2 * S.pr_hid * nl, torch.float32)
            self.conv(W.pr_aln_all, xin.sl(S.d_txt, S.style_pr), gb, what="pr.aln")
            g_at, gs = (lambda i: gb.ptr + 2 * S.pr_hid * i * 4), 2 * S.pr_hid * nl
        else:
            gb = self.act("pr.gb", B, T, 2 * S.pr_hid, torch.float32)
            g_at, gs = (lambda i: gb.ptr), 2 * S.pr_hid
        for i in range(nl):
            self.lstm(W.pr_de[i], xin, hout, f"pr.de{i}", lens=lens)
            if gs == 2 * S.pr_hid:
                self.conv(W.pr_aln[i], xin.sl(S.d_txt, S.style_pr), gb, what=f"pr.aln{i}")
            self.rowln(hout, Act(xin.t, 0, S.pr_hid), G=g_at(i), gs=gs, Bt=g_at(i) + S.pr_hid * 4,
                       bs=gs, gdiv=1, gadd=1.0, what=f"pr.adaln{i}")
        ov = None
        if durations is not None:
            if (durations.device.type != "cpu" and durations.dtype == torch.int32 and durations.is_contiguous() and
                    tuple(durations.shape) == (B, T)):
                ov = durations  # (read only by the alignment and the durations kernel: no device copy, r06)
            else:
                ov = self.buf("pr.dur_ov", (B, T), torch.int32)
                if durations.device.type == "cpu":
                    ov.copy_(durations.to(torch.int32))
                elif durations.data_ptr() != ov.data_ptr():
                    ov.copy_(durations)
        return xin, ov

    def duration_head(self, d: Act, ov=None, hd: Act = None, text_lens=None, controls: RowControls = None) -> dict:
        """a6: duration LSTM + projection + durations kernel (sum of the bin sigmoids, rounded, >= 1; the given
        durations `ov` override it); hd: the duration LSTM's output when already run (lstm_pair)
        -> dict(dur int32 [B, T], dsum, logits, d).  text_lens: the LSTM resets at each row's end, dur and dsum
        are 0 past it.  controls: row b's speed r_b makes a predicted duration max(1, rint(dsum / r_b))
        (stzs_dur_args.rate); dsum stays the raw sum, given durations and padding tokens are as without it."""
        S, W = self.spec, self.W
        B, T = d.B, d.T
        lens = self.text_lens(text_lens, B, T)
        if hd is None:
            hd = self.act("pr.hd", B, T, S.pr_hid, self.adt)
            self.lstm(W.pr_dur_lstm, d, hd, "pr.dur_lstm", lens=lens)
        logits = self.act("pr.logits", B, T, S.dur_bins, torch.float32)
        self.conv(W.pr_dur_proj, hd, Act(logits.t, 0, S.dur_bins), what="pr.dur_proj")
        dur = self.buf("pr.dur", (B, T), torch.int32)
        dsum = self.buf("pr.dsum", (B, T), torch.float32)
        a = L.DurArgs()
        a.logits, a.override_dur, a.dur, a.dsum = logits.ptr, (ov.data_ptr() if ov is not None else None), \
            dur.data_ptr(), dsum.data_ptr()
        a.ldl, a.bsl, a.B, a.T, a.nbins = logits.ld, logits.bs, B, T, S.dur_bins
        a.lens = lens.data_ptr() if lens is not None else None
        if controls is not None and controls.rows(B).use_rate:
            a.rate = controls.rate.data_ptr()
        self._call(self.lib.stzs_durations, a, "durations")
        return dict(dur=dur, dsum=dsum, logits=logits, d=d)

    def prosody_frames(self, h_txt: Act, codes: torch.Tensor, d: Act, dur: torch.Tensor, T40: int,
                       extra: dict = None, pair_dur=False, text_lens=None, ragged_frames=False,
                       controls: RowControls = None) -> dict:
        """a7-a8 for a batch sharing T40 aligned frames: alignment, gathers, shared LSTM, F0 / N curves.
        pair_dur: the duration LSTM over d runs in the shared LSTM's launch (its output as "_hd"), with the rows'
        text_lens when the text is ragged (the frames are not: one T40).
        ragged_frames: T40 is the padded width and row b holds its own frame count, the sum of its durations -- the
        alignment's total[b], read on the device by every later kernel (no host sync), returned as "frame_lens".
        Row b's idx / en / aligned text rows / F0[b, :2 T_b] / N[b, :2 T_b] are those of the row alone at T40 = T_b;
        past it idx is -1, en and the aligned text rows are zeros, F0 / N finite and unspecified (prosody_rows cuts
        the rows of one frame count out for decode()).  Not on a blk_splitk engine (NotImplementedError).
        controls: their pitch_shift, as f0n_predictor (dur already holds the rows' rates)."""
        if ragged_frames:
            self._check_ragged_frames()
        S, W = self.spec, self.W
        B, T = h_txt.B, h_txt.T
        pin = S.pr_in
        idx = self.buf("pr.idx", (B, T40), torch.int32)
        total = self.buf("pr.total", (B,), torch.int32)
        a = L.AlignArgs()
        a.dur, a.idx, a.total, a.B, a.T, a.T40 = dur.data_ptr(), idx.data_ptr(), total.data_ptr(), B, T, T40
        self._call(self.lib.stzs_alignment, a, "alignment")
        en = self.act("pr.en", B, T40, pin, self.adt)
        self.gather(d, idx, en, pin)
        enc_in = self.act("dec.enc_in", B, T40, S.d_txt + 2, self.dec_dt)
        if h_txt.t.dtype != enc_in.t.dtype:  # precise decoder on bf16 text rows: gather, then widen to fp32
            e16 = self.act("dec.enc_in16", B, T40, S.d_txt)
            self.gather(h_txt, idx, e16, S.d_txt)
            self.copy2d(e16, enc_in, T40, S.d_txt)
        else:
            self.gather(h_txt, idx, enc_in, S.d_txt)
        hd = self.act("pr.hd", B, T, S.pr_hid, self.adt) if pair_dur else None
        F0, Nn = self.f0n_predictor(en, codes,
                                    dur_rec=(W.pr_dur_lstm, d, hd, "pr.dur_lstm", text_lens) if pair_dur else None,
                                    frame_lens=total if ragged_frames else None, controls=controls)
        out = dict(extra or {}, dur=dur, idx=idx, T40=T40, en=en, asr_buf=enc_in, d=d, F0=F0, N=Nn)
        if ragged_frames:
            out["frame_lens"] = total
        if pair_dur:
            out["_hd"] = hd
        return out

    def f0n_predictor(self, en: Act, codes: torch.Tensor, dur_rec=None, frame_lens=None,
                      controls: RowControls = None):
        """a8: shared BiLSTM over the aligned frames, then per branch (F0, N) three AdaIN residual blocks (the
        middle one x2 upsampling) and a 1x1 projection.  en [B, T40, pr_in] bf16 -> F0, N fp32 [B, 2 T40].
        frame_lens (int32 [B] device tensor, ragged frames): row b holds frame_lens[b] frames of the T40; the LSTM
        resets at its end, statistics / block convs / upsampling take the lengths (stzs_conv_args.t_lens, ...), so
        F0[b, :2 frame_lens[b]] and N likewise are those of the row alone; past it they are finite, unspecified.
        Statistics are finalised where they are produced (no pro_part, no deferral): the shared xs statistics are
        complete on the current stream before the F0 || N fork.
        controls: row b's pitch factor float32(2 ** (p_b / 12)) multiplies F0[b, :] in one stzs_row_scale launch right
        behind pr.f0_proj (on the F0 branch's stream), before anything reads F0; N is untouched; no launch when the
        shift is absent or 0 everywhere."""
        fl = frame_lens
        mul = controls.mul if controls is not None and controls.rows(en.B).use_pitch else None
        if fl is not None:
            self._check_ragged_frames()
        S, W = self.spec, self.W
        B, T40 = en.B, en.T
        xs = self.act("pr.xs", B, T40, S.pr_hid, self.adt)
        if dur_rec is None:
            self.lstm(W.pr_shared, en, xs, "pr.shared", lens=fl)
        else:  # dur_rec = (lw, x, y, key, text_lens | None): the duration LSTM beside it, one launch
            self.lstm_pair((W.pr_shared, en, xs, "pr.shared", fl), dur_rec)
        sg = self.mean_rows(codes, S.style_ac, S.style_pr, "pr.sg")
        ng = W.pr_norm
        gbp = self.buf("pr.gbn", (B, ng.total), torch.float32)
        self.conv(ng.lin, Act(sg[:, None]), Act(gbp[:, None]), rows=self._rows_z(ng.lin), what="pr.norms")
        T80 = 2 * T40
        F0 = self.buf("pr.F0", (B, T80, 1), torch.float32)
        Nn = self.buf("pr.N", (B, T80, 1), torch.float32)
        c0, c1, c2 = S.f0n_ch

        s0 = self.stats(xs, "pr.xs.s1", fl)  # (both branches' first AdaIN normalise xs: its statistics once, r06)
        if self.f0n_pair and self.blk_splitk and not self._fork_on("f0n"):
            # (r06) the two branches in lockstep, each block's two convs of both branches as one launch pair
            # (stzs_conv1d_group -> conv_mfma_pair / splitk_epi_pair): same bits as branch after branch
            ys = {br: (self.act(f"pr.{br}.y0", B, T40, c0, self.adt), self.act(f"pr.{br}.y1", B, T80, c1, self.adt),
                       self.act(f"pr.{br}.y2", B, T80, c2, self.adt)) for br in ("f0", "n")}
            ins = {"f0": xs, "n": xs}
            for i in range(3):
                self._blk_pair([(W.pr_blk[f"pr.{br}{i}"], ins[br], ys[br][i], f"pr.{br}{i}", s0 if i == 0 else None)
                                for br in ("f0", "n")], ng, gbp, self.adt)
                ins = {br: ys[br][i] for br in ("f0", "n")}
            for br, out in (("f0", F0), ("n", Nn)):
                self.conv(W.pr_blk[f"pr.{br}_proj"], ys[br][2], Act(out, 0, 1), what=f"pr.{br}_proj")
                if br == "f0" and mul is not None:
                    self.row_scale(out, mul)
            return F0[:, :, 0], Nn[:, :, 0]

        def branch(br, out):
            y0 = self.act(f"pr.{br}.y0", B, T40, c0, self.adt)
            y1 = self.act(f"pr.{br}.y1", B, T80, c1, self.adt)
            y2 = self.act(f"pr.{br}.y2", B, T80, c2, self.adt)
            self.blk(W.pr_blk[f"pr.{br}0"], xs, y0, ng, gbp, f"pr.{br}0", self.adt, s1=s0, flens=fl)
            self.blk(W.pr_blk[f"pr.{br}1"], y0, y1, ng, gbp, f"pr.{br}1", self.adt, flens=fl)
            self.blk(W.pr_blk[f"pr.{br}2"], y1, y2, ng, gbp, f"pr.{br}2", self.adt, flens=fl, fmul=2)
            self.conv(W.pr_blk[f"pr.{br}_proj"], y2, Act(out, 0, 1), what=f"pr.{br}_proj")
            if br == "f0" and mul is not None:
                self.row_scale(out, mul)
        self.fork("f0n", lambda: branch("f0", F0), lambda: branch("n", Nn))
        return F0[:, :, 0], Nn[:, :, 0]

    def resample(self, x: torch.Tensor, sr_in: int, sr_out: int, lens=None, lens_mul=1, dtype=torch.float32, out=None,
                 out_lens=None):
        """sample-rate conversion on the device, one launch (stzs_resample): x fp32 [B, N] at sr_in ->
        (y [B, ceil(N L / M)] at sr_out, out_lens int32 [B] on the device).  lens: the rows' own lengths (times
        lens_mul samples) -- B host integers (checked: each product in [0, N]; uploaded) or an int32 [B] device tensor
        (trusted: the kernel clamps) -- row b is then the conversion of its first n_b samples alone, exact zeros from
        out_lens[b] = ceil(n_b L / M) on.  dtype: torch.float32 or torch.int16 (16-bit PCM).  sr_in == sr_out is the
        identity filter (fp32 -> PCM16).  Bad rates raise ValueError before any launch."""
        rs = RS.resampler(self.device, sr_in, sr_out)
        x = x.to(self.device, torch.float32)
        if lens is not None and not (isinstance(lens, torch.Tensor) and lens.device.type != "cpu"):
            t = torch.as_tensor(lens)
            if t.dim() != 1 or t.shape[0] != x.shape[0] or t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f"resample: lens must be {x.shape[0]} integers (one per row)")
            if t.numel() and (int(t.min()) < 0 or int(t.max()) * int(lens_mul) > x.shape[1]):
                raise ValueError(f"resample: lens x {lens_mul} must lie in [0, {x.shape[1]}], got {t.tolist()}")
            lens = t.to(torch.int32).to(self.device)
        self.launches += 1
        return rs(x, lens, lens_mul, dtype, out, out_lens)

    def _ref_in(self, ref_wav, ref_sr, ref_lens, prompt_idx):
        """the reference at the model's rate: with ref_sr another rate, ref_wav [B|1, N] is converted on the device
        first (one launch, before the encoders fork) and its lengths mapped -- host ref_lens are mapped with out_len,
        checked at the model's rate as ref_lens() checks them, and uploaded once (at the source rate: the kernel maps
        them on the device); device ref_lens are trusted and mapped by the kernel, no sync -> (ref_wav, ref_lens)"""
        S = self.spec
        if ref_sr is None or int(ref_sr) == S.sr or ref_wav is None or prompt_idx is not None:
            if ref_sr is not None:
                RS.ratio(int(ref_sr), S.sr)
            return ref_wav, ref_lens
        rs = RS.resampler(self.device, int(ref_sr), S.sr)
        x = ref_wav.to(self.device, torch.float32)
        B, N = x.shape
        n24 = rs.out_len(N)
        lens = None
        if ref_lens is not None:
            if isinstance(ref_lens, torch.Tensor) and ref_lens.device.type != "cpu":
                if ref_lens.dtype != torch.int32 or tuple(ref_lens.shape) != (B,) or not ref_lens.is_contiguous():
                    raise ValueError(f"device ref_lens must be a contiguous int32 [{B}] tensor")
                lens = ref_lens
            else:
                host = torch.as_tensor(ref_lens)
                if host.dim() != 1 or host.shape[0] != B or host.dtype.is_floating_point or host.dtype == torch.bool:
                    raise ValueError(f"ref_lens must be {B} integers (one per reference row)")
                if B and (int(host.min()) < 1 or int(host.max()) > N):
                    raise ValueError(f"ref_lens must lie in [1, {N}] at {ref_sr} Hz, got {host.tolist()}")
                check_ref_lens([rs.out_len(int(v)) for v in host.tolist()], B, n24, S.mel_nfft)
                lens = self.buf("rs.ref_lens_in", (B,), torch.int32)
                lens.copy_(host.to(torch.int32))
        y = self.buf("rs.ref", (B, n24), torch.float32)
        ol = self.buf("rs.ref_lens", (B,), torch.int32)
        self.launches += 1
        rs(x, lens, 1, torch.float32, y, ol)
        return y, (None if lens is None else ol)

    def _wav_out(self, wav, out_sr, out_dtype, frame_lens=None):
        """the decoder's waveform at the caller's rate and type (one launch; None, None: the waveform itself):
        frame_lens (ragged): row b converted as alone on its 600 frame_lens[b] samples, exact zeros behind"""
        S = self.spec
        if out_sr is None and out_dtype is None:
            return wav
        sr = S.sr if out_sr is None else int(out_sr)
        dt = torch.float32 if out_dtype is None else out_dtype
        rs = RS.resampler(self.device, S.sr, sr)
        if dt not in (torch.float32, torch.int16):
            raise ValueError("out_dtype must be torch.float32 or torch.int16")
        if sr == S.sr and dt == torch.float32:
            return wav
        B, N = wav.shape
        y = self.buf("rs.out", (B, rs.out_len(N)), dt)
        ol = self.buf("rs.out_lens", (B,), torch.int32)
        self.launches += 1
        rs(wav, frame_lens, S.frame40 if frame_lens is not None else 1, dt, y, ol)
        return y

    def _check_out(self, out_sr, out_dtype):
        """the output rate and type of synth() / synth_stream(), checked before any launch (ValueError)"""
        if out_sr is not None:
            RS.ratio(self.spec.sr, int(out_sr))
        if out_dtype not in (None, torch.float32, torch.int16):
            raise ValueError("out_dtype must be torch.float32 or torch.int16")

    def row_scale(self, x: torch.Tensor, mul: torch.Tensor):
        """x [B, T, 1] fp32 (a curve per utterance) *= mul[b], in place: one launch (stzs_row_scale)"""
        a = L.RowScaleArgs()
        a.x, a.mul, a.ld, a.bs, a.B, a.T = x.data_ptr(), mul.data_ptr(), x.stride(1), x.stride(0), x.shape[0], x.shape[1]
        self._call(self.lib.stzs_row_scale, a, "row_scale")

    def gather(self, x: Act, idx, y: Act, Cn):
        a = L.GatherArgs()
        a.x, a.idx, a.y = x.t.data_ptr(), idx.data_ptr(), y.t.data_ptr()
        a.ldx, a.bsx, a.ldy, a.bsy = x.ld, x.bs, y.ld, y.bs
        a.B, a.Tsrc, a.Tdst, a.C, a.xc0, a.yc0, a.dtype = x.B, x.T, y.T, Cn, x.c0, y.c0, x.dt
        self._call(self.lib.stzs_gather_rows, a, "gather")

    def blk(self, bw, x: Act, out: Act, ng, gb: torch.Tensor, key, dt=torch.bfloat16, s1=None, flens=None, fmul=1):
        """AdainResBlk1d: out = (conv2(act(AdaIN(conv1(up(act(AdaIN(x))))))) + sc(x)) / sqrt 2.
        s1: x's statistics when the caller already has them (self.stats(x, ...)).
        flens (int32 [B] device tensor, ragged frames): utterance b's x holds flens[b] * fmul rows (fmul 2 behind the
        upsampling block); statistics, the k3 convs and the upsampling take the lengths, the 1x1 shortcut needs none
        (its rows past an utterance's end are never read as a residual)."""
        s1 = s1 if s1 is not None else self.stats(x, key + ".s1", flens, fmul)
        r, s2 = self._blk_conv1(bw, x, s1, ng, gb, key, dt, flens=flens, fmul=fmul)
        self._blk_conv2(bw, r, s2, self._blk_shortcut(bw, x, key, dt), out, ng, gb, key, dt, flens=flens,
                        fmul=2 if bw.up else fmul)
        return out

    def _blk_pair(self, items, ng, gb: torch.Tensor, dt):
        """blk() for two independent blocks of the same shape (items: (bw, x, out, key, s1) each), advanced side by
        side: statistics, upsampling and shortcuts one block after the other, each conv pair collected into one
        stzs_conv1d_group call (the library pairs the batch-1 DEEP split-K convs, else runs them in turn)."""
        st = [s1 if s1 is not None else self.stats(x, key + ".s1") for _, x, _, key, s1 in items]
        refs = [m.ref for m, _, _ in st if isinstance(m, _StatPtr) and not m.ref.done]
        if len(refs) == len(items) and len({id(r) for r in refs}) == len(refs) and all(it[0].up for it in items):
            self._finalize_group(refs)  # (the upsampling blocks' dwup reads mean / rstd: both finalised in one launch)
        grp = []
        rs = [self._blk_conv1(bw, x, s1, ng, gb, key, dt, collect=grp) for (bw, x, _, key, _), s1 in zip(items, st)]
        self._launch_group(grp, "blk.conv1")
        res = [self._blk_shortcut(bw, x, key, dt) for bw, x, _, key, _ in items]
        grp = []
        for (bw, _, out, key, _), (r, s2), rr in zip(items, rs, res):
            self._blk_conv2(bw, r, s2, rr, out, ng, gb, key, dt, collect=grp)
        self._launch_group(grp, "blk.conv2")

    def _blk_weights(self, bw, dt):
        """-> (conv1, conv2, shortcut | None, split-K slices) of an AdaIN block: in the batch-1 engine the
        generic-layout copies split-K (blk_splitk), else the register-direct convs"""
        sk = self.blk_splitk if dt == torch.bfloat16 else 0
        pick = lambda s, c: s if (sk and s is not None) else c
        return pick(bw.conv1s, bw.conv1), pick(bw.conv2s, bw.conv2), \
            (None if bw.sc is None else pick(bw.scs, bw.sc)), sk

    def _blk_conv1(self, bw, x: Act, s1, ng, gb: torch.Tensor, key, dt, collect=None, flens=None, fmul=1):
        """a block's conv1 over act(AdaIN(x)) -- in an upsampling block over the x2 depthwise ConvTranspose of it
        (stzs_adain_dwup) -- with its output's statistics fused -> (r, (mean, rstd, stat_bs) of r)"""
        c1, _, _, sk = self._blk_weights(bw, dt)
        m1, r1, sb1 = s1
        off1, n1 = ng.offsets[bw.name + ".norm1"]
        gb1, gbs = gb.data_ptr() + off1 * 4, ng.total
        To = 2 * x.T if bw.up else x.T
        r = self.act(key + ".r", x.B, To, bw.dout, dt)
        kw = dict(pad=1, stats_key=key + ".s2", splitk=sk, collect=collect, what=key + ".conv1")
        if flens is not None:  # (conv1 of an upsampling block reads the doubled rows)
            assert not (bw.up and fmul != 1), key
            kw.update(t_lens=flens, t_lens_mul=2 if bw.up else fmul)
        if not bw.up:
            return r, self.conv(c1, x, r, pro=(m1, r1, sb1, gb1, gbs, n1), pro_act=L.ACT_LEAKY, pro_slope=0.2, **kw)[1]
        u = self.act(key + ".u", x.B, To, bw.din, dt)
        a = L.DwupArgs()
        a.x, a.y, a.mean, a.rstd, a.gb = x.ptr, u.ptr, m1.data_ptr(), r1.data_ptr(), gb1
        a.w, a.wb = self.W.t(bw.pool_w).data_ptr(), self.W.t(bw.pool_b).data_ptr()
        a.ldx, a.bsx, a.ldy, a.bsy, a.stat_bs, a.gb_bs, a.gb_beta_off = x.ld, x.bs, u.ld, u.bs, sb1, gbs, n1
        a.B, a.T, a.C, a.slope, a.dtype = x.B, x.T, bw.din, 0.2, x.dt
        a.lens = flens.data_ptr() if flens is not None else None
        self._call(self.lib.stzs_adain_dwup, a, key + ".dwup")
        return r, self.conv(c1, u, r, **kw)[1]

    def _blk_shortcut(self, bw, x: Act, key, dt) -> Act:
        """a block's residual input: its 1x1 shortcut conv of x, or x itself"""
        _, _, sc, sk = self._blk_weights(bw, dt)
        if sc is None:
            return x
        scb = self.act(key + ".sc", x.B, x.T, bw.dout, dt)
        return self.conv(sc, x, scb, splitk=sk, what=key + ".sc")

    def _blk_conv2(self, bw, r: Act, s2, res: Act, out: Act, ng, gb: torch.Tensor, key, dt, collect=None, flens=None,
                   fmul=1):
        """a block's conv2 over act(AdaIN(r)), plus the residual, / sqrt 2 -> out"""
        _, c2, _, sk = self._blk_weights(bw, dt)
        m2, r2, sb2 = s2
        off2, n2 = ng.offsets[bw.name + ".norm2"]
        self.conv(c2, r, out, pad=1, pro=(m2, r2, sb2, gb.data_ptr() + off2 * 4, ng.total, n2), pro_act=L.ACT_LEAKY,
                  pro_slope=0.2, res=res, res_tdiv=2 if bw.up else 1, alpha=1.0 / math.sqrt(2.0), splitk=sk,
                  collect=collect, what=key + ".conv2", **({} if flens is None else dict(t_lens=flens, t_lens_mul=fmul)))

    # ------------------------------------------------------------------ (c) decoder
    def decode(self, pro: dict, codes: torch.Tensor, seeds, istft=True, frame_lens=None, trace=None,
               rows=None) -> torch.Tensor:
        """a9-a13: decoder pre-blocks, generator, conv_post + iSTFT.  pro: asr_buf (aligned text features in the
        decoder input buffer), F0 / N [B, T80], T40 -> wav fp32 [B, 600 T40] (or conv_post rows, istft=False).
        frame_lens (int32 [B] device tensor, the ragged decoder): row b holds frame_lens[b] of the T40
        frames -- the alignment's totals, predict_prosody(ragged_frames=True)["frame_lens"] -- and is computed as
        alone at T40 = frame_lens[b]: wav[b, :600 frame_lens[b]] are those bits, the tail exact zeros; no host sync.
        rows: frame_rows(frame_lens, T40) where the caller made them already (synth_stream hands their last array to the
        streaming iSTFT).  trace (a dict): the stages' activations (generator())."""
        if frame_lens is None:
            # the harmonic source depends on F0 only: forkable beside the decoder pre-blocks (fork site "src")
            (gen_in, gbd), har = self.fork("src", lambda: self.decoder_pre(pro, codes),
                                           lambda: self.sine_gen(pro["F0"], seeds))
            if trace is not None:
                trace["gen_in"] = gen_in
            return self.generator(gen_in, pro["F0"], seeds, gbd, trace=trace, istft=istft, har=har)
        self._check_ragged_decoder()
        if rows is None:
            rows = self.frame_rows(frame_lens, pro["T40"])  # (on the current stream, before the fork: both branches wait)
        (gen_in, gbd), har = self.fork("src", lambda: self.decoder_pre(pro, codes, frame_lens),
                                       lambda: self.sine_gen(pro["F0"], seeds, rows[0]))
        if trace is not None:
            trace["gen_in"] = gen_in
        return self.generator(gen_in, pro["F0"], seeds, gbd, trace=trace, istft=istft, har=har, rows=rows)

    def frame_rows(self, frame_lens: torch.Tensor, T40: int):
        """the ragged decoder's row counts, from the rows' 40-fps frame counts (int32 [B] on the device, clamped into
        [1, T40]) in ONE launch (stzs_frame_rows) -> int32 [B] device tensors: [0] the 80-fps rows 2 T_b (the decoder
        output, the harmonic source's frames), [1 + i] the rows of generator stage i, 2 T_b prod r_j (+ 1 behind the
        last stage's reflection pad: conv_post's rows and the iSTFT frame count)."""
        S = self.spec
        B = frame_lens.shape[0]
        assert frame_lens.dtype == torch.int32 and frame_lens.shape == (B,) and frame_lens.is_contiguous()
        n = 1 + len(S.up_rates)
        out = self.buf("gen.frame_rows", (n, B), torch.int32)
        a = L.FrameRowsArgs()
        a.lens, a.out, a.B, a.T, a.n = frame_lens.data_ptr(), out.data_ptr(), B, int(T40), n
        m = 2
        a.mul[0] = m
        for i, r in enumerate(S.up_rates):
            m *= r
            a.mul[1 + i], a.add[1 + i] = m, int(i == len(S.up_rates) - 1)
        self._call(self.lib.stzs_frame_rows, a, "frame_rows")
        return [out[k] for k in range(n)]

    def _check_ragged_decoder(self):
        """the ragged decoder runs where every generator conv takes a form with length-aware kernels
        (stzs_conv_args.t_lens_rows = 1).  Not the latency engine's split-K blocks.  A precise decoder (precise=True
        or precise_decoder=True, fp32 rows): every generator conv has split-operand weights, so it routes to the mrfx or
        the conv_x3 form, which both take the lengths -- an fp32 decoder whose convs would run on
        conv_f32 is refused.  The bf16 decoder: a spec whose MRF convs and ConvTransposes are on the register-direct
        form and whose conv_post is on the narrow form (SPEC_V0; not SPEC_TINY's generic convs).  Before any launch."""
        self._check_ragged_frames()
        W = getattr(self, "W", None)  # (no packed weights: no form can be vouched for)
        if self.dec_dt != torch.bfloat16:
            gen = [] if W is None else \
                [lw[c] for st in W.rb for res in st for lw in res for c in ("c1", "c2")] + list(W.ups) + [W.conv_post]
            if not gen or not all(getattr(cw, "wx3", None) is not None or getattr(cw, "fx3", None) is not None
                                  for cw in gen):
                raise NotImplementedError("ragged decoder: an fp32 decoder takes per-row lengths on the split-operand "
                                          "forms (mrfx, conv_x3) only, not on conv_f32 (STZS_CONV_W_F32)")
            return
        ok = W is not None and all(getattr(lw[c], "frag32", False) and lw["k"] in (3, 7, 11)
                                   for st in W.rb for res in st for lw in res for c in ("c1", "c2"))
        ok = ok and all(getattr(u, "frag32", False) and u.ci_pad // 128 <= 4 for u in W.ups)
        ok = ok and getattr(W.conv_post, "narrow32", False)
        if not ok:
            raise NotImplementedError("ragged decoder: a bf16 generator's MRF convs and ConvTransposes must take the "
                                      "register-direct form and conv_post the narrow form (generic-path bf16 convs "
                                      "do not take per-row lengths; neither do conv_f32 or the blk_splitk blocks)")

    def dec_style(self, codes: torch.Tensor) -> torch.Tensor:
        """every AdaIN gamma / beta of the decoder from the pooled acoustic codes: ONE GEMM -> [B, total] fp32."""
        S, W = self.spec, self.W
        B = codes.shape[0]
        sa = self.mean_rows(codes, 0, S.style_ac, "dec.sa")
        ng = W.dec_norm
        gbd = self.buf("dec.gbn", (B, ng.total), torch.float32)
        self.conv(ng.lin, Act(sa[:, None]), Act(gbd[:, None]), rows=self._rows_z(ng.lin), what="dec.norms")
        return gbd

    def decoder_pre(self, pro: dict, codes: torch.Tensor, frame_lens=None):
        """a9: F0 / N stride-2 convs, asr_res, the encode block and the four decode blocks (1024 channels,
        the last one x2 upsampling) -> (generator input [B, T80, dec_out], decoder AdaIN gammas/betas).
        frame_lens (int32 [B] device tensor, ragged frames): the blocks take the rows' frame counts (blk(flens=...):
        statistics, k3 convs, the upsampling); the F0 / N stride-2 convs need none -- output frame T_b - 1 reads F0 / N
        rows 2 T_b - 3 .. 2 T_b - 1, inside the row -- and asr_res and the shortcuts are row-local.  Rows at and past
        a row's end are finite and unspecified."""
        S, W = self.spec, self.W
        enc_in, F0, Nn, T40 = pro["asr_buf"], pro["F0"], pro["N"], pro["T40"]
        B = enc_in.B
        T80 = 2 * T40
        gbd = self.dec_style(codes)
        ng = W.dec_norm
        dcat = S.dec_enc + 2 + S.dec_asr_res
        dt = self.dec_dt
        cats = [self.act("dec.catA", B, T40, dcat, dt), self.act("dec.catB", B, T40, dcat, dt)]
        cF, cN = S.dec_enc + S.dec_asr_res, S.dec_enc + S.dec_asr_res + 1
        for j, cat in enumerate(cats):
            a = L.F0nArgs()
            a.f0, a.n = F0.data_ptr(), Nn.data_ptr()
            a.wf, a.wn = W.t(W.dec_f0).data_ptr(), W.t(W.dec_n).data_ptr()
            a.y0, a.y1 = cat.t.data_ptr(), (enc_in.t.data_ptr() if j == 0 else None)
            a.ldf, a.ldy0, a.bsy0, a.ldy1, a.bsy1 = F0.stride(0), cat.ld, cat.bs, enc_in.ld, enc_in.bs
            a.B, a.T80, a.cf0, a.cn0, a.cf1, a.cn1, a.dtype = B, T80, cF, cN, S.d_txt, S.d_txt + 1, cat.dt
            assert enc_in.t.dtype == cat.t.dtype
            self._call(self.lib.stzs_f0n_down, a, "f0n_down")
            self.conv(W.dec_asr_res, Act(enc_in.t, 0, S.d_txt), cat.sl(S.dec_enc, S.dec_asr_res), what="asr_res")
        self.blk(W.dec_blk["dec.encode"], Act(enc_in.t, 0, S.d_txt + 2), cats[0].sl(0, S.dec_enc), ng, gbd, "dec.encode",
                 dt, flens=frame_lens)
        src = 0
        for i in range(3):
            self.blk(W.dec_blk[f"dec.decode{i}"], Act(cats[src].t, 0, dcat), cats[1 - src].sl(0, S.dec_enc), ng, gbd,
                     f"dec.decode{i}", dt, flens=frame_lens)
            src = 1 - src
        gen_in = self.act("dec.gen_in", B, T80, S.dec_out, dt)
        self.blk(W.dec_blk["dec.decode3"], Act(cats[src].t, 0, dcat), gen_in, ng, gbd, "dec.decode3", dt,
                 flens=frame_lens)
        return gen_in, gbd

    def sine_gen(self, F0: torch.Tensor, seeds, lens=None) -> Act:
        """a10: NSF harmonic source from F0 [B, T80] (SineGen: fp64 frame-rate phase prefix, counter-RNG noise,
        Linear(9->1) + tanh) and its n_fft-point STFT (real | imag) -> har [B, Tf, har_ch] (csrc/source.hip).
        lens (int32 [B] device tensor, the ragged decoder): row b's 80-fps frames; its har rows past its own frame
        count are zeros (stzs_source_args.lens)."""
        S, W = self.spec, self.W
        B, T80 = F0.shape[0], F0.shape[1]
        N = T80 * S.hop
        Tf = N // S.istft_hop + 1
        nh = S.harmonic_num + 1
        if isinstance(seeds, torch.Tensor) and seeds.device.type != "cpu":
            sd = seeds.to(torch.int32)
        else:
            skey = ("seeds", tuple(int(v) for v in seeds))
            sd = self._consts.get(skey)
            if sd is None:  # uploaded once per distinct seed list (graph-capture safe afterwards)
                host = torch.as_tensor(np.asarray(seeds, dtype=np.uint32).view(np.int32).copy())
                sd = self._consts[skey] = host.to(self.device)
        pref = self.buf("gen.pref", (B, nh, T80), torch.float32)
        # row pitch = the noise convs' padded K (32): the 1x1 noise conv then takes the LDS-DMA GEMM path
        dt = self.dec_dt
        # rows rounded up to a multiple of the first stage's noise-conv stride (zero past Tf): the buffer then reads as
        # whole super-rows (engine.upsample's super-row noise conv); the Act is the view of its Tf frames
        hb = self.buf("gen.har", (B, self._har_rows(Tf), _rup(S.har_ch, 32)), dt, zero=True)
        har = Act(hb[:, :Tf], 0, S.har_ch)
        a = L.SourceArgs()
        a.f0, a.seeds, a.merge_w, a.prefix, a.har = F0.data_ptr(), sd.data_ptr(), W.t(W.src_merge).data_ptr(), \
            pref.data_ptr(), har.ptr
        a.ldf, a.ldh, a.bsh = F0.stride(0), har.ld, har.bs
        a.B, a.T80, a.hop, a.n_fft, a.hop_s, a.nh = B, T80, S.hop, S.n_fft, S.istft_hop, nh
        a.sr, a.sine_amp, a.noise_std, a.voiced_thr = float(S.sr), S.sine_amp, S.noise_std, S.voiced_threshold
        a.har_dtype = har.dt
        if lens is not None:
            a.lens = lens.data_ptr()
        self._call(self.lib.stzs_harmonic_source, a, "harmonic_source",  # F0 in, prefix, STFT rows out
                   cost=(0, B * T80 * 4 * (1 + 2 * nh) + B * Tf * S.har_ch * har.t.element_size()))
        return har

    def _har_rows(self, Tf: int) -> int:
        """rows allocated for Tf harmonic-source frames: a multiple of the stage-0 noise-conv stride"""
        s = math.prod(self.spec.up_rates[1:]) if len(self.spec.up_rates) > 1 else 1
        return _rup(Tf, s)

    def upsample(self, x: Act, har: Act, i: int, rows=None) -> Act:
        """a11: generator stage i's noise conv of the harmonic features + LeakyReLU(0.1) -> polyphase
        ConvTranspose1d(k = 2 r, s = r) (+ ReflectionPad(1,0) on the last stage) + the noise conv as residual.
        rows (int32 [B] device tensor, the ragged decoder): the rows of x each utterance holds -- the ConvTranspose
        takes them (t_lens_rows 1); the noise convs take no length: they have no prologue and the harmonic-source rows
        past an utterance's end are zeros, the padding they see at its end alone."""
        rg = {} if rows is None else dict(t_lens=rows, t_lens_rows=1)
        S, W = self.spec, self.W
        B = x.B
        n_up = len(S.up_rates)
        r, k = S.up_rates[i], S.up_kernels[i]
        c = S.gen_ch[i]
        last = i == n_up - 1
        Tcur = x.T
        Tn = Tcur * r + (1 if last else 0)
        dt = self.dec_dt
        xu = self.act(f"gen.x{i}", B, Tn, c, dt)
        nzw = self.W.ups_nz[i] if (self.ups_noise_fused and i < len(self.W.ups_nz)) else None
        if nzw is not None and dt == torch.bfloat16 and har.ld >= 32:
            # the 1x1 noise conv fused into the ConvTranspose (csrc/ups.hip STZS_CONV_UPS_NOISE): one more K-step per
            # column tile on the harmonic-source rows; its output never goes through HBM
            self.conv(nzw, x, xu, pro_act=L.ACT_LEAKY, pro_slope=0.1, ups_pad=(k - r) // 2, T_final=Tcur * r,
                      refl=1 if last else 0, res=Act(har.t, 0, har.ld), flags=L.CONV_UPS_NOISE,
                      gate=self._t(nzw.nz32).data_ptr(), what=f"ups{i}", **rg)
            return xu
        xsrc = self.act(f"gen.xsrc{i}", B, Tn, c, dt)
        sup = W.noise_sup[i] if (not last and i < len(W.noise_sup)) else None
        sf0 = int(np.prod(S.up_rates[i + 1:])) if not last else 1
        rows_alloc = har.bs // har.ld  # rows of the buffer behind the Tf-frame view (zero past Tf)
        if (sup is not None and self.noise_super and har.dt == L.BF16 and har.bs % (sf0 * har.ld) == 0 and
                rows_alloc // sf0 >= Tn + 1 and sf0 * har.ld == sup.Ci and har.t.stride(1) == har.ld):
            # the strided noise conv on SUPER-ROWS (weights.noise_super_weights): the harmonic-source buffer read as
            # [B, rows / s, s * 32] is a k3 stride-1 conv over 192 channels -> the register-direct kernel (mrfv.hip)
            # instead of a stride-6 conv staging 6 rows of 64 B per output row
            hs = har.t.as_strided((B, rows_alloc // sf0, sf0 * har.ld), (har.bs, sf0 * har.ld, 1))
            self.conv(sup, Act(hs), xsrc, pad=1, T_out=Tn, what=f"noise_conv{i}")
        elif not last:
            # (T_out explicit: the harmonic buffer holds rows past the Tf frames -- zeros, rounded up for the super-row
            # view -- so har.T would over-count the output rows)
            self.conv(W.noise_conv[i], har.sl(0, S.har_ch), xsrc, stride=sf0, pad=(sf0 + 1) // 2, T_out=Tn,
                      what=f"noise_conv{i}")
        else:
            self.conv(W.noise_conv[i], har.sl(0, S.har_ch), xsrc, T_out=Tn, what=f"noise_conv{i}")
        self.conv(W.ups[i], x, xu, pro_act=L.ACT_LEAKY, pro_slope=0.1, ups_pad=(k - r) // 2, T_final=Tcur * r,
                  refl=1 if last else 0, res=xsrc, what=f"ups{i}", **rg)
        return xu

    def conv_post(self, x: Act, rows=None, out: Act = None) -> Act:
        """LeakyReLU(0.01) + conv_post (128 -> 22, k7) -> fp32 rows [B, Tf, 22] (log-magnitude | phase argument).
        rows (int32 [B] device tensor, the ragged decoder): the rows of x each utterance holds.
        out: the caller's fp32 rows [B, Tf, >= 22] instead of the engine's buffer (the ragged chunked decoder's)."""
        S, W = self.spec, self.W
        post = out if out is not None else self.act("gen.post", x.B, x.T, S.har_ch, torch.float32)
        assert post.B == x.B and post.T == x.T and post.t.dtype == torch.float32
        self.conv(W.conv_post, x, Act(post.t, 0, S.har_ch), pad=3, pro_act=L.ACT_LEAKY, pro_slope=0.01,
                  what="conv_post", **({} if rows is None else dict(t_lens=rows, t_lens_rows=1)))
        return post

    def istft(self, post: Act, lens=None) -> torch.Tensor:
        """a13: exp / sin spectrum, 20-point irfft, Hann overlap-add (hop 5), window-envelope normalisation.
        lens (int32 [B] device tensor, the ragged decoder): each utterance's frames; the samples past its own last one
        are zeros (stzs_istft_args.lens)."""
        S = self.spec
        B, Tcur = post.B, post.T
        Nout = (Tcur - 1) * S.istft_hop
        wav = self.buf("gen.wav", (B, Nout), torch.float32)
        a = L.IstftArgs()
        a.post, a.wav, a.ldp, a.bsp, a.bsw = post.ptr, wav.data_ptr(), post.ld, post.bs, Nout
        a.B, a.Tf, a.n_fft, a.hop_s = B, Tcur, S.n_fft, S.istft_hop
        if lens is not None:
            a.lens = lens.data_ptr()
        self._call(self.lib.stzs_istft, a, "istft", cost=(0, B * Tcur * S.har_ch * 4 + B * Nout * 4))
        return wav

    def generator(self, x: Act, F0: torch.Tensor, seeds, gbd, trace=None, istft=True, har: Act = None, rows=None,
                  post_out: Act = None):
        """a10-a13: harmonic source, per stage the noise conv + ConvTranspose up-sampling and the MRF, then
        conv_post and the iSTFT.  har: precomputed harmonic-source features (the chunked decoder's window slice).
        rows (frame_rows(), the ragged decoder): the row counts of x ([0]) and of every stage's output ([1 + i]).
        post_out: conv_post's rows go there (conv_post(out=...))."""
        S, W = self.spec, self.W
        ng = W.dec_norm
        rw = (lambda k: None) if rows is None else (lambda k: rows[k])
        if har is None:
            har = self.sine_gen(F0, seeds, rw(0))
        if trace is not None:
            trace["har"] = har
        for i in range(len(S.up_rates)):
            xu = self.upsample(x, har, i, rw(i))
            if trace is not None:
                trace[f"mrf_in{i}"] = xu
            x = self.mrf(xu, i, gbd, ng, rw(1 + i))
            if trace is not None:
                trace[f"mrf_out{i}"] = x
        post = self.conv_post(x, rw(len(S.up_rates)), post_out)
        if trace is not None:
            trace["post"] = post
        if not istft:
            return post
        return self.istft(post, rw(len(S.up_rates)))

    def _istft_chunk(self, rows_ptr, ldp, bsp, B, f0, Fc, fin, wav, tails, i, lens=None, post_off=None):
        """one streaming-iSTFT launch: conv_post frames [f0, f0 + Fc) at rows_ptr (row pitch ldp, batch stride bsp,
        fp32) -> samples [n0, n1) of wav [B, Nout], the 3-frame tail carried in the ping-pong buffers.  -> (n0, n1)
        lens / post_off (int32 [B] device tensors, ragged streaming): each row's absolute frame count and the row of
        rows_ptr + b * bsp its chunk frames start at (stzs_istft_stream_args)."""
        S = self.spec
        n0, n1 = C.c_int64(), C.c_int64()
        halo = self.lib.stzs_istft_stream_span(f0, Fc, fin, S.n_fft, S.istft_hop, C.byref(n0), C.byref(n1))
        L.check(min(halo, 0), "istft_stream_span")
        assert halo <= 8
        a = L.IstftStreamArgs()
        a.post = rows_ptr
        a.tail_in = tails[i % 2].data_ptr() if f0 > 0 else None
        a.tail_out = tails[(i + 1) % 2].data_ptr() if not fin else None
        a.wav = wav.data_ptr() + n0.value * 4
        a.ldp, a.bsp, a.bsw, a.ldt = ldp, bsp, wav.shape[1], tails[0].shape[2]
        a.B, a.f0, a.Fc, a.final_chunk, a.n_fft, a.hop_s = B, f0, Fc, fin, S.n_fft, S.istft_hop
        if lens is not None:
            a.lens = lens.data_ptr()
        if post_off is not None:
            a.post_off = post_off.data_ptr()
        self._call(self.lib.stzs_istft_stream, a, "istft_stream")
        return n0.value, n1.value

    @staticmethod
    def chunk_windows(T40: int, chunk: int, halo: int):
        """the chunked decoder's schedule (oracle/stzs_ref.py chunk_windows): chunk i owns aligned frames
        [i chunk, min((i + 1) chunk, T40)) and is decoded over a window of fixed length W = min(chunk + 2 halo, T40)
        starting at clamp(a - halo, 0, T40 - W).  -> [(a, b, wa, wb)]"""
        W = min(chunk + 2 * halo, T40)
        out = []
        for a in range(0, T40, chunk):
            wa = min(max(0, a - halo), T40 - W)
            out.append((a, min(a + chunk, T40), wa, wa + W))
        return out

    @staticmethod
    def ragged_chunk_windows(frame_lens, chunk: int, halo: int):
        """the ragged chunked decoder's schedule (host arithmetic): row b of the batch keeps its OWN schedule
        chunk_windows(T_b, chunk, halo); batch chunk k, owning the aligned frames [k chunk, (k + 1) chunk), holds the
        rows that still have a window there (k chunk < T_b).  -> one list per batch chunk, ceil(max T_b / chunk) of
        them, of (row, (a, b, wa, wb)) in row order."""
        per_row = [StyleTTSZS.chunk_windows(int(T_b), chunk, halo) for T_b in frame_lens]
        n = max((len(w) for w in per_row), default=0)
        return [[(b, w[k]) for b, w in enumerate(per_row) if k < len(w)] for k in range(n)]

    def decode_chunked(self, pro: dict, codes: torch.Tensor, seeds, chunk: int, halo: int, batch_windows=True,
                       max_pass_rows: int = 64, frame_lens=None):
        """configs[4] CHUNKED streaming decoder (oracle/stzs_ref.py decode_chunked): each chunk of `chunk` aligned
        frames is decoded over its fixed-length window (chunk_windows) -- pre-blocks and generator on the window alone,
        AdaIN with WINDOW-local InstanceNorm statistics -- on the slice of the whole utterance's harmonic-source
        features (global phase prefix and noise counters); its own conv_post frames go through the streaming iSTFT with
        the carried tail.  The first chunk's window is decoded alone (its audio is ready after one window's decode);
        with batch_windows every later window is then decoded in ONE pass, the windows as the rows of one batch
        (window-major, [window][utterance]): every decoder kernel is batch-invariant (per-utterance tiles and
        statistics), so this is bit-identical to decoding them one by one (batch_windows=False), in 3 passes' worth of
        launches instead of one per chunk.  A pass holds at most max(B, max_pass_rows) window rows (windows x utterances):
        a pass's audio is ready only when the whole pass is decoded and its activations scale with its rows, so at large
        B or long targets the later windows go in several passes (time to the second chunk ~ one pass's decode; peak
        activation memory ~ max_pass_rows windows).  Yields (first_sample, wav chunk [B, n]) views of one [B, 600 T40]
        buffer.
        frame_lens (ragged streaming): the rows' frame counts T_b as HOST integers -- a list or CPU
        tensor, each in [1, T40], range-checked before any launch; a device tensor is read back once (one host sync:
        the window schedule is made on the host).  Row b keeps the schedule chunk_windows(T_b, chunk, halo) and its
        samples [0, 600 T_b) are the bits of this call on the row alone at T40 = T_b, exact zeros from there; the
        chunks tile [0, 600 max T_b) (_decode_chunked_ragged)."""
        if frame_lens is not None:
            self._check_ragged_decoder()
            yield from self._decode_chunked_ragged(pro, codes, seeds, int(chunk), int(halo), batch_windows,
                                                   max_pass_rows, frame_lens)
            return
        S = self.spec
        enc_in, F0, Nn, T40 = pro["asr_buf"], pro["F0"], pro["N"], pro["T40"]
        B = enc_in.B
        fpf = S.frame40 // S.istft_hop
        har = self.sine_gen(F0, seeds)
        Nout = T40 * S.frame40
        wav = self.buf("gen.wav_chunked", (B, Nout), torch.float32)
        ncol = _rup(S.n_fft + 2, 4)
        tails = [self.buf("gen.ctail0", (B, 8, ncol), torch.float32), self.buf("gen.ctail1", (B, 8, ncol), torch.float32)]
        dt = self.dec_dt
        wins = self.chunk_windows(T40, chunk, halo)
        Wn = wins[0][3] - wins[0][2]
        Tfw = fpf * Wn + 1
        if batch_windows:
            per = max(1, max_pass_rows // max(B, 1))  # windows per pass after the first
            rest = list(range(1, len(wins)))
            groups = [[0]] + [rest[i:i + per] for i in range(0, len(rest), per)]
        else:
            groups = [[k] for k in range(len(wins))]
        groups = [g for g in groups if g]
        F0c, Nc = F0.contiguous(), Nn.contiguous()
        cdt = L.F32 if codes.dtype == torch.float32 else L.BF16
        for ks in groups:
            nw = len(ks)
            Bw = nw * B
            enc_w = self.act("dec.enc_in_w", Bw, Wn, S.d_txt + 2, dt)
            har_w = Act(self.buf("gen.har_w", (Bw, self._har_rows(Tfw), har.ld), dt, zero=True)[:, :Tfw], 0, S.har_ch)
            F0w = self.buf("dec.F0w", (Bw, 2 * Wn), torch.float32)
            Nw = self.buf("dec.Nw", (Bw, 2 * Wn), torch.float32)
            cw_ = codes if nw == 1 else self.buf("dec.codes_w", (Bw,) + tuple(codes.shape[1:]), codes.dtype)
            esz, hsz = enc_in.t.element_size(), har.t.element_size()
            for b in range(B):
                # runs of windows whose starts are `chunk` apart: one strided copy per run and tensor
                i = 0
                while i < nw:
                    j = i + 1
                    while j < nw and wins[ks[j]][2] - wins[ks[j - 1]][2] == chunk:
                        j += 1
                    wa, cnt = wins[ks[i]][2], j - i
                    row = i * B + b  # window-major rows of the batch
                    self._copy_rows(enc_in.t.data_ptr() + (b * enc_in.bs + wa * enc_in.ld) * esz, enc_in.ld,
                                    chunk * enc_in.ld, enc_w.t.data_ptr() + row * enc_w.bs * esz, enc_w.ld,
                                    B * enc_w.bs, cnt, Wn, S.d_txt, enc_in.dt, enc_w.dt)
                    self._copy_rows(har.t.data_ptr() + (b * har.bs + fpf * wa * har.ld) * hsz, har.ld,
                                    fpf * chunk * har.ld, har_w.t.data_ptr() + row * har_w.bs * hsz, har_w.ld,
                                    B * har_w.bs, cnt, Tfw, S.har_ch, har.dt, har_w.dt)
                    for src, dst in ((F0c, F0w), (Nc, Nw)):
                        self._copy_rows(src.data_ptr() + (b * src.stride(0) + 2 * wa) * 4, 2 * Wn, 2 * chunk,
                                        dst.data_ptr() + row * 2 * Wn * 4, 2 * Wn, B * 2 * Wn, cnt, 1, 2 * Wn,
                                        L.F32, L.F32)
                    i = j
                if nw > 1:  # every window of utterance b takes its codes (source block stride 0)
                    Lc, Dc = codes.shape[1], codes.shape[2]
                    self._copy_rows(codes.data_ptr() + b * codes.stride(0) * codes.element_size(), Dc, 0,
                                    cw_.data_ptr() + b * Lc * Dc * cw_.element_size(), Dc, B * Lc * Dc, nw, Lc, Dc,
                                    cdt, cdt)
            gen_in, gbd = self.decoder_pre(dict(asr_buf=enc_w, F0=F0w, N=Nw, T40=Wn), cw_)
            post = self.generator(gen_in, F0w, seeds, gbd, istft=False, har=har_w)
            for i, k in enumerate(ks):
                a0, b0, wa, _ = wins[k]
                fin = int(b0 == T40)
                r0 = fpf * (a0 - wa)
                n0, n1 = self._istft_chunk(post.ptr + (i * B * post.bs + r0 * post.ld) * 4, post.ld, post.bs, B,
                                           fpf * a0, fpf * (b0 - a0) + fin, fin, wav, tails, k)
                yield n0, wav[:, n0:n1]

    def _decode_chunked_ragged(self, pro, codes, seeds, chunk, halo, batch_windows, max_pass_rows, frame_lens):
        """decode_chunked on a ragged batch (ragged_chunk_windows).  The harmonic source is computed once, ragged.  A
        pass holds only the (utterance, window) rows that exist, utterance-major, at the width of its longest window,
        and is decoded through the ragged decoder on the window lengths (frame_rows, decoder_pre(frame_lens),
        generator(rows)): a window is computed as alone, with window-local statistics.  Each batch chunk is ONE
        stzs_istft_stream launch over all B rows: lens = 120 T_b + 1 finalises a row by its own count, post_off points
        a row at its own window's frames, a finished row gets zeros.  A row whose T_b is a multiple of `chunk` has its
        last frame (120 T_b) read by the NEXT batch chunk's launch, from the window that computed it: where that
        window belongs to an earlier pass, the frame is kept in a spare row in front of the pass's conv_post rows.
        The pass's two int32 tables (window lengths, post_off per chunk) are built on the host and uploaded once."""
        enc_in, F0, Nn, T40 = pro["asr_buf"], pro["F0"], pro["N"], int(pro["T40"])
        B = enc_in.B
        Tb = check_frame_lens(frame_lens, B, T40)  # (before any launch; a device tensor: the one host read)
        S, dev = self.spec, self.device
        if isinstance(frame_lens, torch.Tensor) and frame_lens.device.type != "cpu":
            fl = frame_lens.to(torch.int32).contiguous()
        else:
            fl = torch.tensor(Tb, dtype=torch.int32).to(dev)
        fpf = S.frame40 // S.istft_hop
        assert fpf == 2 * math.prod(S.up_rates)
        full = self.frame_rows(fl, T40)
        har = self.sine_gen(F0, seeds, full[0])
        lens_abs = full[-1].clone()  # fpf T_b + 1 (the passes' frame_rows reuse the buffer)
        Tm = max(Tb)
        wav = self.buf("gen.wav_chunked", (B, T40 * S.frame40), torch.float32)
        ncol = _rup(S.n_fft + 2, 4)
        tails = [self.buf("gen.ctail0", (B, 8, ncol), torch.float32), self.buf("gen.ctail1", (B, 8, ncol), torch.float32)]
        dt = self.dec_dt
        sched = self.ragged_chunk_windows(Tb, chunk, halo)
        nck = len(sched)
        if batch_windows:
            per = max(1, max_pass_rows // max(B, 1))  # batch chunks per pass after the first
            rest = list(range(1, nck))
            groups = [[0]] + [rest[i:i + per] for i in range(0, len(rest), per)]
        else:
            groups = [[k] for k in range(nck)]
        groups = [g for g in groups if g]
        # per pass: its rows, utterance-major -- (utterance, [(batch chunk, window)])
        passes = []
        for ks in groups:
            byrow = {}
            for k in ks:
                for b, w in sched[k]:
                    byrow.setdefault(b, []).append((k, w))
            passes.append(sorted(byrow.items()))
        ldp = _rup(S.har_ch, 8)
        nsp = _rup(B, 4)  # spare rows in front: utterance b's last frame, carried from an earlier pass
        cap = max(sum(len(v) for _, v in p) * (fpf * max(w[3] - w[2] for _, v in p for _, w in v) + 1) for p in passes)
        pw = self.buf("gen.post_w", (nsp + cap, ldp), torch.float32, zero=True)
        F0c, Nc = F0.contiguous(), Nn.contiguous()
        cdt = L.F32 if codes.dtype == torch.float32 else L.BF16
        esz, hsz = enc_in.t.element_size(), har.t.element_size()
        last_row = {}  # utterance -> row of pw that holds its frame fpf T_b, where the next pass's first launch reads it
        for ks, rows_p in zip(groups, passes):
            Bw = sum(len(v) for _, v in rows_p)
            Wn = max(w[3] - w[2] for _, v in rows_p for _, w in v)
            Tfw = fpf * Wn + 1
            # ---- the host tables of the pass: window lengths [Bw], then post_off [len(ks)][B]
            wl, ridx, r = [], {}, 0
            for b, v in rows_p:
                for k, w in v:
                    wl.append(w[3] - w[2])
                    ridx[(k, b)] = r
                    r += 1
            offs = []
            for k in ks:
                for b in range(B):
                    if (k, b) in ridx:
                        a0, _, wa, _ = dict(sched[k])[b]
                        offs.append(nsp + ridx[(k, b)] * Tfw + fpf * (a0 - wa))
                    elif Tb[b] == chunk * k:  # its last frame is this launch's first
                        if (k - 1, b) in ridx:
                            offs.append(nsp + ridx[(k - 1, b)] * Tfw + fpf * min(chunk + 2 * halo, Tb[b]))
                        else:
                            assert b in last_row
                            offs.append(b)  # (its spare row, filled below)
                    else:
                        offs.append(0)  # finished: nothing is read
            tab = torch.tensor(wl + offs, dtype=torch.int32).to(dev)
            wl_d = tab[:Bw]
            # ---- window rows: zeros past a window's own rows (the harmonic-source rows there are the noise convs' padding)
            enc_w = self.act("dec.enc_in_w", Bw, Wn, S.d_txt + 2, dt)
            hb = self.buf("gen.har_w", (Bw, self._har_rows(Tfw), har.ld), dt, zero=True)
            F0w = self.buf("dec.F0w", (Bw, 2 * Wn), torch.float32, zero=True)
            Nw = self.buf("dec.Nw", (Bw, 2 * Wn), torch.float32, zero=True)
            for t in (enc_w.t, hb, F0w, Nw):
                t.zero_()
            har_w = Act(hb[:, :Tfw], 0, S.har_ch)
            whole = Bw == B and all(len(v) == 1 for _, v in rows_p)  # every utterance once: its codes as they are
            cw_ = codes if whole else self.buf("dec.codes_w", (Bw,) + tuple(codes.shape[1:]), codes.dtype)
            row = 0
            for b, v in rows_p:
                Wb = v[0][1][3] - v[0][1][2]  # (one window length per utterance)
                nw = len(v)
                i = 0
                while i < nw:  # runs of windows whose starts are `chunk` apart: one strided copy per run and tensor
                    j = i + 1
                    while j < nw and v[j][1][2] - v[j - 1][1][2] == chunk:
                        j += 1
                    wa, cnt = v[i][1][2], j - i
                    self._copy_rows(enc_in.t.data_ptr() + (b * enc_in.bs + wa * enc_in.ld) * esz, enc_in.ld,
                                    chunk * enc_in.ld, enc_w.t.data_ptr() + (row + i) * enc_w.bs * esz, enc_w.ld,
                                    enc_w.bs, cnt, Wb, S.d_txt, enc_in.dt, enc_w.dt)
                    self._copy_rows(har.t.data_ptr() + (b * har.bs + fpf * wa * har.ld) * hsz, har.ld,
                                    fpf * chunk * har.ld, har_w.t.data_ptr() + (row + i) * har_w.bs * hsz, har_w.ld,
                                    har_w.bs, cnt, fpf * Wb + 1, S.har_ch, har.dt, har_w.dt)
                    for src, dst in ((F0c, F0w), (Nc, Nw)):
                        self._copy_rows(src.data_ptr() + (b * src.stride(0) + 2 * wa) * 4, 2 * Wb, 2 * chunk,
                                        dst.data_ptr() + (row + i) * 2 * Wn * 4, 2 * Wb, 2 * Wn, cnt, 1, 2 * Wb,
                                        L.F32, L.F32)
                    i = j
                if not whole:  # every window of utterance b takes its codes (source block stride 0)
                    Lc, Dc = codes.shape[1], codes.shape[2]
                    self._copy_rows(codes.data_ptr() + b * codes.stride(0) * codes.element_size(), Dc, 0,
                                    cw_.data_ptr() + row * Lc * Dc * cw_.element_size(), Dc, Lc * Dc, nw, Lc, Dc,
                                    cdt, cdt)
                row += nw
            # ---- the carried last frames move before conv_post overwrites the rows they lie in
            for b, src in last_row.items():
                self._copy_rows(pw.data_ptr() + src * ldp * 4, ldp, 0, pw.data_ptr() + b * ldp * 4, ldp, 0, 1, 1, ldp,
                                L.F32, L.F32)
            rows = self.frame_rows(wl_d, Wn)
            gen_in, gbd = self.decoder_pre(dict(asr_buf=enc_w, F0=F0w, N=Nw, T40=Wn), cw_, wl_d)
            post = Act(pw[nsp:nsp + Bw * Tfw].view(Bw, Tfw, ldp), 0, S.har_ch)
            self.generator(gen_in, F0w, seeds, gbd, istft=False, har=har_w, rows=rows, post_out=post)
            # an utterance that ends with this pass's last batch chunk, on the chunk boundary: the next pass reads its
            # last frame
            last_row = {b: nsp + ridx[(v[-1][0], b)] * Tfw + fpf * (v[-1][1][3] - v[-1][1][2]) for b, v in rows_p
                        if Tb[b] == chunk * (ks[-1] + 1) and ks[-1] + 1 < nck}
            for i, k in enumerate(ks):
                a0 = chunk * k
                b0 = min(a0 + chunk, Tm)
                fin = int(b0 == Tm)
                n0, n1 = self._istft_chunk(pw.data_ptr(), ldp, 0, B, fpf * a0, fpf * (b0 - a0) + fin, fin, wav, tails,
                                           k, lens_abs, tab[Bw + i * B:Bw + (i + 1) * B])
                yield n0, wav[:, n0:n1]

    def istft_stream(self, post: Act, chunk_frames: int, lens=None):
        """iSTFT of conv_post frames [B, Tf, 22] in chunks of `chunk_frames` frames,
        the 3-frame tail carried between chunks (ping-pong buffers).  Yields (n0, wav[:, n0:n1]) as each
        chunk is enqueued; the views are slices of one [B, Nout] buffer, so no chunk overwrites another,
        and their concatenation is bit-identical to the whole-utterance iSTFT.
        lens (int32 [B] device tensor, ragged streaming): each row's iSTFT frames -- the last array of
        frame_rows().  The chunk spans stay those of the padded Tf; row b's samples below (lens[b] - 1) hop_s are the
        bits of istft(lens=...) -- of the row alone --, exact zeros from there, each row finalised by its own count in
        whatever chunk its last samples fall into.  No host sync."""
        S = self.spec
        B, Tf = post.B, post.T
        Nout = (Tf - 1) * S.istft_hop
        wav = self.buf("gen.wav_stream", (B, Nout), torch.float32)
        ncol = _rup(S.n_fft + 2, 4)
        tails = [self.buf("gen.tail0", (B, 8, ncol), torch.float32), self.buf("gen.tail1", (B, 8, ncol), torch.float32)]
        f0, i = 0, 0
        while f0 < Tf:
            Fc = min(chunk_frames, Tf - f0)
            if 0 < Tf - f0 - Fc < 2:  # fold a 1-frame remainder (Tf = 600*T40/5 + 1) into this chunk
                Fc = Tf - f0
            n0, n1 = self._istft_chunk(post.ptr + f0 * post.ld * 4, post.ld, post.bs, B, f0, Fc, int(f0 + Fc == Tf),
                                       wav, tails, i, lens)
            yield n0, wav[:, n0:n1]
            f0 += Fc
            i += 1

    def _launch_group(self, args, what):
        """the collected stzs_conv_args (conv(collect=...)) as ONE stzs_conv1d_group call"""
        arr = (L.ConvArgs * len(args))(*args)
        rc = self.lib.stzs_conv1d_group(arr, len(args), self.stream())
        if rc < 0:
            L.check(rc, what)
        self.launches += rc

    def _finalize_group(self, refs):
        """the statistics of up to three collected convs finalised in one launch (stzs_chan_stats_final_group)"""
        arr = (L.StatsArgs * len(refs))()
        for s, r in zip(arr, refs):
            r.final_args(s)
        assert len({r.chunk_rows for r in refs}) == 1
        self._raw(self.lib.stzs_chan_stats_final_group, "chan_stats_final_group", arr, len(refs), refs[0].chunk_rows)
        for r in refs:
            r.done = True

    def _rb_c1(self, lw, x: Act, y: Act, st, gbd, ng, stats_key, collect=None, **kw):
        """a resblock layer's first conv (dilated) over Snake(AdaIN(x)), st = x's (mean, rstd, stat_bs), with y's
        statistics fused -> (mean, rstd, stat_bs) of y"""
        k, dil = lw["k"], lw["dil"]
        o1, c1 = ng.offsets[lw["n1"]]
        return self.conv(lw["c1"], x, y, pad=dil * (k - 1) // 2, dil=dil,
                         pro=(*st, gbd.data_ptr() + o1 * 4, ng.total, c1), pro_act=L.ACT_SNAKE, pro_alpha=lw["a1"],
                         stats_key=stats_key, collect=collect, what="rb.c1", **kw)[1]

    def _rb_c2(self, lw, x: Act, y: Act, st, res: Act, gbd, ng, **kw):
        """a resblock layer's second conv over Snake(AdaIN(x)) + res; kw: the caller's epilogue / statistics /
        collect arguments -> conv()'s result"""
        o2, c2 = ng.offsets[lw["n2"]]
        return self.conv(lw["c2"], x, y, pad=(lw["k"] - 1) // 2, pro=(*st, gbd.data_ptr() + o2 * 4, ng.total, c2),
                         pro_act=L.ACT_SNAKE, pro_alpha=lw["a2"], res=res, what="rb.c2", **kw)

    def _mrf_trio(self, x: Act, i, gbd, ng):
        """mrf() with the three resblocks (k 3 / 7 / 11) advanced layer by layer side by side: each layer's c1 convs in
        ONE launch (stzs_conv1d_group -> mrfv_trio at small batch), their statistics in one, the non-last c2 convs and
        their statistics likewise; the last layer's c2 convs stay one after the other (each adds the previous
        resblocks' sum, acc_in).  Per-resblock buffers; every value bit-identical to mrf()'s order."""
        S, W = self.spec, self.W
        B, T, c = x.B, x.T, x.C
        dt = x.t.dtype
        nk = len(S.rb_kernels)
        xs = self.act(f"gen.xs{i}", B, T, c, dt)
        t1 = [self.act(f"gen.t1_{i}.{j}", B, T, c, dt) for j in range(nk)]
        bufs = [(self.act(f"gen.ba{i}.{j}", B, T, c, dt), self.act(f"gen.bb{i}.{j}", B, T, c, dt)) for j in range(nk)]
        mx, rx, sb = self.stats(x, f"gen.sx{i}")
        cur, cm, cr = [x] * nk, [mx] * nk, [rx] * nk
        nl = len(W.rb[i][0])
        for m in range(nl):
            grp = []
            st1 = [self._rb_c1(res[m], cur[j], t1[j], (cm[j], cr[j], sb), gbd, ng, f"gen.st{i}.{j}", collect=grp)
                   for j, res in enumerate(W.rb[i])]
            self._launch_group(grp, "rb.c1")
            self._finalize_group([st[0].ref for st in st1])
            if m == nl - 1:  # xs = c2 / nk + cur (+ xs): the resblocks' sum in resblock order, one launch each
                for j, res in enumerate(W.rb[i]):
                    self._rb_c2(res[m], t1[j], xs, (*st1[j][:2], sb), cur[j], gbd, ng, alpha=1.0 / nk,
                                acc_in=(xs if j > 0 else None), beta=1.0)
                break
            grp = []
            outs = [bufs[j][0] if cur[j] is not bufs[j][0] else bufs[j][1] for j in range(nk)]
            st2 = [self._rb_c2(res[m], t1[j], outs[j], (*st1[j][:2], sb), cur[j], gbd, ng,
                               stats_key=f"gen.sc{i}.{j}.{m % 2}", collect=grp)[1] for j, res in enumerate(W.rb[i])]
            self._launch_group(grp, "rb.c2")
            self._finalize_group([st[0].ref for st in st2])
            for j in range(nk):
                cur[j], (cm[j], cr[j], _) = outs[j], st2[j]
        return xs

    def _mrf_trio_on(self, x: Act, i) -> bool:
        """the side-by-side schedule applies: small batch, no timer running (its collected convs are not timed), and
        the stage's resblocks are the k 3 / 7 / 11 trio of equal depth the library groups"""
        rb = self.W.rb[i]
        return (self.mrf_trio and self.timer is None and x.B <= 4 and tuple(self.spec.rb_kernels) == (3, 7, 11) and
                len({len(res) for res in rb}) == 1 and all(r["k"] == k for res, k in zip(rb, (3, 7, 11)) for r in res))

    def mrf(self, x: Act, i, gbd, ng, rows=None):
        """a12: the stage's resblocks (k 3 / 7 / 11) summed / 3.  rows (int32 [B] device tensor, the ragged decoder):
        the rows of x each utterance holds -- the statistics and every Snake conv take them (t_lens_rows 1), each
        conv's fused statistics finalised where they are produced with the same array (no deferral, no trio): the
        uniform path's bits row for row."""
        S, W = self.spec, self.W
        rg = {} if rows is None else dict(t_lens=rows, t_lens_rows=1)
        if rows is None and self._mrf_trio_on(x, i):
            return self._mrf_trio(x, i, gbd, ng)
        B, T, c = x.B, x.T, x.C
        dt = x.t.dtype
        xs = self.act(f"gen.xs{i}", B, T, c, dt)
        bufA = self.act(f"gen.ba{i}", B, T, c, dt)
        bufB = self.act(f"gen.bb{i}", B, T, c, dt)
        t1 = self.act(f"gen.t1_{i}", B, T, c, dt)
        mx, rx, sb = self.stats(x, f"gen.sx{i}", rows)
        nk = len(S.rb_kernels)
        for j, res in enumerate(W.rb[i]):
            cur, cm, cr = x, mx, rx
            for m, lw in enumerate(res):
                tm, tr, _ = self._rb_c1(lw, cur, t1, (cm, cr, sb), gbd, ng, f"gen.st{i}", **rg)
                last = m == len(res) - 1
                out = xs if last else (bufA if cur is not bufA else bufB)
                r2 = self._rb_c2(lw, t1, out, (tm, tr, sb), cur, gbd, ng, alpha=(1.0 / nk) if last else 1.0,
                                 acc_in=(xs if (last and j > 0) else None), beta=1.0,
                                 stats_key=None if last else f"gen.sc{i}.{m % 2}", **rg)
                if not last:
                    _, (cm, cr, _) = r2
                    cur = out
        return xs

    # ------------------------------------------------------------------ end to end
    def twin(self) -> "StyleTTSZS":
        """a second engine on the SAME packed weights with its own buffer cache: two twins can synthesize
        two utterance batches concurrently on two streams (their graphs replay side by side, so one batch's
        latency-bound phases -- LSTM recurrences, statistics, small GEMMs -- overlap the other's convs)."""
        t = object.__new__(StyleTTSZS)
        t.__dict__.update(self.__dict__)
        t._bufs, t._retired, t._consts, t._side, t._branch, t.launches, t.timer = {}, [], {}, {}, "", 0, None
        t._depth = 0
        t.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        return t

    def encode_inputs(self, tokens, ref_wav, prompt_idx=None, text_lens=None, ref_lens=None, voices=None):
        """text encoder || prompt encoder (independent; forked when branch_streams) -> (h_txt, prompt codes).
        ref_lens: per-row sample counts of a ragged reference batch; host lengths are checked and uploaded here, on
        the current stream, before the fork (the forked prompt branch waits on it).
        voices (VoiceRows; ref_wav None): the prompt branch is one stzs_voice_prompt launch (voice_encode)."""
        if voices is not None:
            self._check_voices(voices, tokens, ref_wav, prompt_idx, ref_lens)
            return self.fork("enc", lambda: self.text_encode(tokens, text_lens), lambda: self.voice_encode(voices))
        ref = None if ref_wav is None else ref_wav.to(self.device)
        if prompt_idx is not None or ref is None:
            ref_lens = None  # (teacher-forced codes: the reference and its lengths are unused)
        else:
            ref_lens = self.ref_lens(ref_lens, ref.shape[0], ref.shape[1])
        return self.fork("enc", lambda: self.text_encode(tokens, text_lens),
                         lambda: self.prompt_encode(ref, prompt_idx, ref_lens))

    def capture(self, fn):
        """Capture `fn()` into one HIP graph.  fn must be replay-safe: device-resident inputs, cached
        buffers (a warm-up call on a side stream allocates them), no host syncs (synth() skips its status
        check while capturing).  -> (CheckedGraph, fn's output); graph.check() raises after a replay whose LSTM
        exchange timed out (the captured kernels OR the flag into this engine's status word)."""
        cur = torch.cuda.current_stream(self.device)
        s = torch.cuda.Stream(self.device)
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            fn()
        cur.wait_stream(s)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn()
        for k, ent in self._bufs.items():
            if isinstance(k, tuple):
                ent[3] = True
        return CheckedGraph(g, self), out

    def _capturing(self) -> bool:
        return torch.cuda.is_current_stream_capturing()

    def synth(self, tokens, ref_wav, steps=2, cfg_scale=1.0, noise=None, durations=None, seeds=None, codes=None,
              n_frames=None, prompt_idx=None, check=True, text_lens=None, ref_lens=None, ragged_frames=False,
              controls: RowControls = None, ref_sr=None, out_sr=None, out_dtype=None, voices=None):
        """tokens int [B, T_txt]; ref_wav fp32 [B|1, N]; noise fp32 [B, L_s, code]; durations int [B, T_txt]
        (host tensor, or device tensor + n_frames: no device sync); seeds: per-utterance source-noise
        seeds; prompt_idx: teacher-forced discrete prompt codes [B|1, L_s, G] (ref_wav then unused).
        text_lens: int [B] (host: range-checked; int32 device tensor: trusted, no sync), each in [1, T_txt] -- a
        ragged batch: row b is computed as alone on its first text_lens[b] tokens (DESIGN.md "Ragged text
        batches").  Without ragged_frames the rows must still share one frame count.
        ragged_frames=True: the rows need not share their frame count -- ragged prosody
        (predict_prosody(ragged_frames=True)) and the ragged decoder (decode(frame_lens=...)) at the padded width of
        the longest row (or n_frames) -> (wav [B, 600 T40], frame_lens int32 [B] on the device): row b is valid to
        600 frame_lens[b], the bits of the row alone, and exact zeros from there.
        ref_lens: int [B|1], one per row of ref_wav (host: range-checked; int32 device tensor: trusted, no sync), each
        in [mel_nfft / 2 + 1, N] -- a ragged reference batch: row b's prompt is computed as alone on
        ref_wav[b, :ref_lens[b]], what lies past it is never read; ignored, as ref_wav is, when
        prompt_idx is given.
        controls (row_controls()): one guidance scale, speaking rate and pitch shift per row -- row b is
        computed as alone with its values; a cfg_scale of theirs replaces the argument; rows of different rates have
        different frame counts (ragged_frames).  Device arrays: a captured synth() replays with what
        RowControls.set() wrote.
        ref_sr: the rate of ref_wav where it is not the model's: converted on the device first (one
        launch); ref_lens then count samples at ref_sr and are mapped to the model's rate (host: checked there;
        device: by the kernel, no sync).  out_sr / out_dtype: the waveform converted to that rate and to torch.int16
        (16-bit PCM) or fp32, one launch behind the decoder: "wav" is at out_sr and the dict gains "sr"; with
        ragged_frames row b is valid to ceil(600 frame_lens[b] out_sr / sr) and exact zeros from there.  All None: no
        launch is added.
        voices (voice_rows()): the speakers as enrolled voices, one or a blend per row -- ref_wav is
        then None and the prompt front end is ONE launch (stzs_voice_prompt); with any of ref_wav, prompt_idx, ref_lens
        or ref_sr: ValueError before any launch.  Device arrays: a captured synth() replays for the speakers
        VoiceRows.set() wrote.
        check: raise RuntimeError if an LSTM exchange of this call timed out (its durations / prosody would be
        wrong) -- one 4-B device read, skipped while a graph is being captured (CheckedGraph.check() then);
        check=False leaves it to the caller (check_status(), or the returned `status` word).
        -> dict(wav=[B, 600*T40], prompt_idx=[B|1, L_s, G], status=int32 [1], ...)"""
        self._check_voices(voices, tokens, ref_wav, prompt_idx, ref_lens, ref_sr)
        if ragged_frames:
            self._check_ragged_decoder()
        self._check_out(out_sr, out_dtype)
        h, prompt, codes, pro, seeds = self._front(tokens, ref_wav, steps, cfg_scale, noise, durations, seeds, codes,
                                                   n_frames, prompt_idx, text_lens, ref_lens, ragged_frames, controls,
                                                   ref_sr, voices)
        wav = self.decode(pro, codes, seeds, frame_lens=pro["frame_lens"] if ragged_frames else None)
        wav = self._wav_out(wav, out_sr, out_dtype, pro["frame_lens"] if ragged_frames else None)
        if check and not self._capturing():
            self.check_status()
        if ragged_frames:
            return wav, pro["frame_lens"]
        out = dict(wav=wav, codes=codes, h_txt=h, prompt=prompt, prompt_idx=self.prompt_idx, status=self.status, **pro)
        if out_sr is not None or out_dtype is not None:
            out["sr"] = self.spec.sr if out_sr is None else int(out_sr)
        return out

    def _front(self, tokens, ref_wav, steps, cfg_scale, noise, durations, seeds, codes, n_frames, prompt_idx,
               text_lens=None, ref_lens=None, ragged_frames=False, controls: RowControls = None, ref_sr=None,
               voices=None):
        """everything before the decoder, shared by synth() and synth_stream(): tokens to the device, text || prompt
        encoders (one prompt broadcast over the batch), style sampling unless codes are given, prosody, default seeds
        -> (h_txt, prompt, codes, pro, seeds); the prompt's discrete codes are in self.prompt_idx"""
        S = self.spec
        dev = self.device
        self._check_voices(voices, tokens, ref_wav, prompt_idx, ref_lens, ref_sr)
        tokens = tokens.to(dev, torch.int32) if tokens.device != dev or tokens.dtype != torch.int32 else tokens
        B = tokens.shape[0]
        text_lens = self.text_lens(text_lens, B, tokens.shape[1])  # (host lengths: checked and uploaded once)
        if ref_sr is not None:  # (a reference at another rate: converted on this stream, before the encoders fork)
            ref_wav, ref_lens = self._ref_in(ref_wav, ref_sr, ref_lens, prompt_idx)
        if voices is not None:
            h, prompt = self.encode_inputs(tokens, None, None, text_lens, None, voices)
        else:
            h, prompt = self.encode_inputs(tokens, ref_wav, prompt_idx, text_lens, ref_lens)
        if prompt.shape[0] == 1 and B > 1:
            pe = self.buf("prompt.bc", (B, S.L_s, S.code_dim), torch.float32)
            pe.copy_(prompt.expand(B, -1, -1))
            prompt = pe
        if codes is None:
            codes = self.sample_style(h, prompt, noise.to(dev, torch.float32), steps, cfg_scale, text_lens, controls)
        pro = self.predict_prosody(h, codes, durations, n_frames, text_lens, ragged_frames, controls)
        return h, prompt, codes, pro, list(range(B)) if seeds is None else seeds

    def synth_stream(self, tokens, ref_wav, steps=2, cfg_scale=1.0, noise=None, durations=None, seeds=None,
                     codes=None, n_frames=None, chunk_s=1.0, prompt_idx=None, check=True, chunked_halo=None,
                     text_lens=None, ref_lens=None, ragged_frames=False, controls: RowControls = None, ref_sr=None,
                     out_sr=None, out_dtype=None, voices=None):
        """configs[4] long-form synthesis with the streaming iSTFT decoder: the text,
        style, prosody and conv stack run over the whole target (AdaIN instance statistics are
        utterance-global), then the waveform is emitted in `chunk_s`-second chunks.  Yields
        (first_sample, wav_chunk [B, n]) device views; their concatenation equals synth()["wav"].
        chunked_halo=H: the CHUNKED decoder instead (decode_chunked: every `chunk_s` chunk decoded over a window of
        +-H aligned frames with window-local statistics -- a different function, parity vs oracle decode_chunked):
        the first chunk is ready after the front and one window's decode.
        ragged_frames=True: the rows need not share their frame count, as synth(ragged_frames=True) --
        ragged prosody, the ragged decoder, the streaming iSTFT on the rows' own frame counts.  The same pairs over the
        padded width; the device frame counts (int32 [B]) are in self.frame_lens from the first yield on: row b is
        valid to 600 frame_lens[b] -- the bits of the row's own stream -- and exact zeros from there.  No host sync is
        added, but for the chunked decoder: it reads the frame counts back once (its window schedule is host work)
        and its chunks tile [0, 600 max frame_lens).
        controls: per-row guidance scale, speaking rate and pitch shift, as synth().
        ref_sr: the reference's rate, as synth().  out_sr / out_dtype: every chunk of either decoder
        goes through one chunked conversion (Resampler.stream: one launch per chunk, and one for the filter's tail
        behind the last); the pairs are (first_out_sample, chunk) at out_sr, contiguous, and their concatenation is
        the bits of the one-shot conversion of the unconverted stream -- with ragged_frames of its rows alone, row b
        valid to ceil(600 frame_lens[b] out_sr / sr).
        voices: the speakers as enrolled voices (ref_wav None), as synth()."""
        self._check_voices(voices, tokens, ref_wav, prompt_idx, ref_lens, ref_sr)
        if ragged_frames:
            self._check_ragged_decoder()
        self._check_out(out_sr, out_dtype)
        _, _, codes, pro, seeds = self._front(tokens, ref_wav, steps, cfg_scale, noise, durations, seeds, codes,
                                              n_frames, prompt_idx, text_lens, ref_lens, ragged_frames, controls, ref_sr,
                                              voices)
        fl = None
        if ragged_frames:
            fl = self.frame_lens = pro["frame_lens"]
        chunks = self._stream_chunks(pro, codes, seeds, chunk_s, chunked_halo, fl)
        if out_sr is not None or out_dtype is not None:
            chunks = self._convert_chunks(chunks, codes.shape[0], fl, out_sr, out_dtype)
        yield from chunks
        if check and not self._capturing():
            self.check_status()

    def _convert_chunks(self, chunks, B, fl, out_sr, out_dtype):
        """the (first_sample, chunk) pairs of a streaming decoder through one chunked sample-rate conversion"""
        S = self.spec
        rs = RS.resampler(self.device, S.sr, S.sr if out_sr is None else int(out_sr))

        def count():
            self.launches += 1
        st = rs.stream(B, fl, S.frame40 if fl is not None else 1, torch.float32 if out_dtype is None else out_dtype,
                       on_launch=count)
        for _, c in chunks:
            j0, y = st.push(c)
            if y.shape[1]:
                yield j0, y
        j0, y = st.push(None, final=True)  # the filter's tail: the outputs whose last taps lie past the signal's end
        if y.shape[1]:
            yield j0, y

    def _stream_chunks(self, pro, codes, seeds, chunk_s, chunked_halo, fl):
        """the (first_sample, chunk) pairs of synth_stream() at the model's rate"""
        S = self.spec
        if chunked_halo is not None:  # the chunked decoder: chunk-local statistics, first audio after one window
            yield from self.decode_chunked(pro, codes, seeds, max(1, int(round(chunk_s * S.sr / S.frame40))),
                                           int(chunked_halo), **({} if fl is None else dict(frame_lens=fl)))
        else:
            frames = max(1, int(round(chunk_s * S.sr / S.istft_hop)))
            if fl is None:
                post = self.decode(pro, codes, seeds, istft=False)
                yield from self.istft_stream(post, frames)
            else:
                rows = self.frame_rows(fl, pro["T40"])
                post = self.decode(pro, codes, seeds, istft=False, frame_lens=fl, rows=rows)
                yield from self.istft_stream(post, frames, lens=rows[-1])


# fork sites of the batch-1 latency engine: the text encoder beside the prompt encoder on a forked branch of the
# captured graph (configs[1] p50 6.06-6.20 -> 5.91 ms, 4 A/B pairs, profiles/r05_m_fork_sites_ab.log); the F0 || N
# fork measured slower (6.19-6.27 vs 6.05-6.18) and stays off.  env STZS_LATENCY_FORKS="" turns it off.
LATENCY_FORKS = frozenset(v for v in os.environ.get("STZS_LATENCY_FORKS", "enc").split(",") if v)


def latency_engine(spec: Spec, packed: PackedModel, device="cuda:0") -> "StyleTTSZS":
    """the batch-1 serving engine bench.py times for the configs[1] p50 (and tests/test_gpu_configs.py checks against
    the oracle): the same packed weights, the denoiser layer linears on the whole-chip small-M form
    (LATENCY_DN_ROWS, csrc/rows.hip) and split-K ffn2 wherever the rows form does not apply (LATENCY_DN_SPLITK);
    with durations given, the duration LSTM paired with the shared LSTM (dur_overlap, on in every engine); the text
    and prompt encoders on forked graph branches (LATENCY_FORKS)."""
    return StyleTTSZS(spec, None, device=device, packed=packed, dn_splitk=LATENCY_DN_SPLITK, dn_rows=LATENCY_DN_ROWS,
                      te_splitk=LATENCY_TE_SPLITK, blk_splitk=LATENCY_BLK_SPLITK, branch_streams=LATENCY_FORKS)


class CheckedGraph:
    """a captured HIP graph of one engine + that engine's LSTM status check (StyleTTSZS.capture).  replay()
    enqueues the graph; check() reads the engine's status word (one 4-B device read, i.e. a sync) and raises if
    any LSTM exchange of the replays since the last check timed out."""

    def __init__(self, graph, eng):
        self.graph, self.eng = graph, eng

    def replay(self):
        self.graph.replay()

    def check(self):
        return self.eng.check_status()


class _OffsetAct(Act):
    """Act whose base pointer is shifted by `off` elements (writes into a row window of a larger buffer)."""

    def __init__(self, base: Act, off: int):
        super().__init__(base.t, base.c0, base.C)
        self._off = off

    @property
    def ptr(self):
        return self.t.data_ptr() + (self.c0 + self._off) * self.t.element_size()
