"""Sample-rate conversion on the device: filter design, the span arithmetic of a streamed
conversion, and the Resampler that holds the device tables of one (sr_in, sr_out) pair and launches stzs_resample.

The kernel is a rational polyphase FIR on caller-supplied tables and knows nothing about windows or sincs; design()
below is where the filter is made: a Kaiser-windowed sinc, `zeros` zero crossings to each side at the lower of the two
rates, everything in float64, the table rounded once to fp32.  With L / M the reduced sr_out / sr_in, output sample
j = q L + p is  sum_k h[p, k] x[q M + o[p] + k].
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L_

MAX_LM = 1024      # include/stzs.h: L, M <= 1024
MAX_K = 512        # K <= 512
MAX_RATIO = 8      # M <= 8 L


def ratio(sr_in: int, sr_out: int):
    """-> (L, M) = (sr_out, sr_in) / gcd, checked against the kernel's limits (ValueError, before any launch)"""
    for name, v in (("sr_in", sr_in), ("sr_out", sr_out)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) <= 0:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    g = math.gcd(int(sr_in), int(sr_out))
    L, M = int(sr_out) // g, int(sr_in) // g
    if L > MAX_LM or M > MAX_LM:
        raise ValueError(f"{sr_in} -> {sr_out} Hz reduces to L / M = {L} / {M}: both must be <= {MAX_LM}")
    if M > MAX_RATIO * L:
        raise ValueError(f"{sr_in} -> {sr_out} Hz decimates by more than {MAX_RATIO}")
    return L, M


def design(sr_in: int, sr_out: int, zeros: int = 32, rolloff: float = 0.945, beta: float = 12.0):
    """-> (L, M, W, K, o int32 [L], h fp32 [L, K4]): the polyphase tables of sr_in -> sr_out.
    s = rolloff min(1, L / M) is the cutoff relative to the input Nyquist, W = ceil(zeros / s) the half width in input
    samples, K = 2 W + 1 taps; phase p reads from o[p] = floor(p M / L) - W, its tap k sits tau = (o[p] + k) - p M / L
    input samples from the output instant:
        h[p, k] = s sinc(s tau) I0(beta sqrt(1 - (tau / (W + 1))^2)) / I0(beta)
    in float64, rounded once to fp32; K4 = K rounded up to a multiple of 4, the padding columns zero.
    sr_in == sr_out is the identity table (L = M = K = 1, W = 0): the fp32 -> PCM16 conversion."""
    L, M = ratio(sr_in, sr_out)
    if L == M:  # == 1
        h = np.zeros((1, 4), np.float32)
        h[0, 0] = 1.0
        return 1, 1, 0, 1, np.zeros(1, np.int32), h
    if zeros < 1 or not (0.0 < rolloff <= 1.0) or beta < 0.0:
        raise ValueError("design: zeros >= 1, 0 < rolloff <= 1, beta >= 0")
    s = rolloff * min(1.0, L / M)
    W = int(math.ceil(zeros / s))
    K = 2 * W + 1
    if K > MAX_K:
        raise ValueError(f"{sr_in} -> {sr_out} Hz needs {K} taps at zeros={zeros}, rolloff={rolloff}: at most {MAX_K}")
    p = np.arange(L, dtype=np.int64)
    o = (p * M) // L - W
    tau = (o[:, None] + np.arange(K, dtype=np.int64)[None, :]).astype(np.float64) - (p * M).astype(np.float64)[:, None] / L
    win = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (tau / (W + 1)) ** 2))) / np.i0(beta)
    h = np.zeros((L, (K + 3) // 4 * 4), np.float32)
    h[:, :K] = (s * np.sinc(s * tau) * win).astype(np.float32)
    return L, M, W, K, o.astype(np.int32), h


def out_len(n: int, L: int, M: int) -> int:
    """output samples of n input samples: ceil(n L / M), in integers"""
    return (int(n) * int(L) + int(M) - 1) // int(M)


def span(n_avail: int, final: bool, n_emitted: int, L: int, M: int, W: int):
    """-> the output range [j0, j1) that can be emitted once the first n_avail input samples exist and n_emitted
    outputs have been emitted: every j whose last tap, input sample floor(j M / L) + W, is below n_avail -- i.e.
    j < (n_avail - W) L / M -- and, with `final` (n_avail is the whole signal), everything up to out_len(n_avail).
    Pure host arithmetic, the analogue of stzs_istft_stream_span."""
    if final:
        j1 = out_len(n_avail, L, M)
    else:
        j1 = out_len(max(int(n_avail) - int(W), 0), L, M)
    j0 = int(n_emitted)
    return j0, max(j0, j1)


_DT = {torch.float32: L_.F32, torch.int16: L_.I16}


class Resampler:
    """the device tables of one (device, sr_in, sr_out) pair and the launches on them.  Built through
    resampler(): one per pair and device."""

    def __init__(self, device, sr_in: int, sr_out: int):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.L, self.M, self.W, self.K, o, h = design(sr_in, sr_out)
        self.o_host, self.h_host = o, h
        self.o = torch.from_numpy(o).to(self.device)
        self.h = torch.from_numpy(h).to(self.device)
        self.lib = L_.load()

    def out_len(self, n: int) -> int:
        return out_len(n, self.L, self.M)

    def _check_x(self, x):
        if x.device != self.device or x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
            raise ValueError(f"resample: x must be an fp32 [B, N] tensor on {self.device} with unit sample stride")

    def _check_lens(self, lens, B):
        if lens is not None and (not isinstance(lens, torch.Tensor) or lens.device != self.device or
                                 lens.dtype != torch.int32 or tuple(lens.shape) != (B,) or not lens.is_contiguous()):
            raise ValueError(f"resample: lens must be a contiguous int32 [{B}] tensor on {self.device}")

    def launch(self, x, x0, n_total, j0, j1, y, lens=None, lens_mul=1, out_lens=None):
        """one stzs_resample launch on the current stream: x [B, n_x] is the window whose first sample has absolute
        index x0 of a signal of n_total samples, y [B, >= j1 - j0] (fp32 or int16) takes the outputs [j0, j1)"""
        if x.shape[0] > 1 and x.stride(0) < x.shape[1]:
            x = x.contiguous()  # (a broadcast row)
        a = L_.ResampleArgs()
        a.x, a.h, a.o, a.y = x.data_ptr(), self.h.data_ptr(), self.o.data_ptr(), y.data_ptr()
        a.lens = None if lens is None else lens.data_ptr()
        a.out_lens = None if out_lens is None else out_lens.data_ptr()
        a.x0, a.n_x, a.bsx, a.n_total = int(x0), x.shape[1], max(x.stride(0), x.shape[1]), int(n_total)
        a.j0, a.j1, a.bsy = int(j0), int(j1), max(y.stride(0), int(j1) - int(j0))
        a.B, a.L, a.M, a.K, a.lens_mul, a.out_dtype = x.shape[0], self.L, self.M, self.K, int(lens_mul), _DT[y.dtype]
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L_.check(self.lib.stzs_resample(C.byref(a), stream), "resample")

    def __call__(self, x, lens=None, lens_mul=1, dtype=torch.float32, out=None, out_lens=None):
        """x fp32 [B, N] at sr_in -> (y [B, out_len(N)] at sr_out, out_lens int32 [B]), one launch.  lens (int32 [B]
        device tensor, times lens_mul: row b's sample count, clamped into [0, N]): row b is the conversion of
        x[b, :n_b] alone, exact zeros from out_lens[b] = out_len(n_b) on.  dtype: torch.float32, or torch.int16 for
        16-bit PCM (clamp(rint(32768 y)), ties to even).  out / out_lens: tensors to write instead of fresh ones."""
        self._check_x(x)
        B, N = x.shape
        if B < 1 or N < 1:
            raise ValueError("resample: empty batch or signal")
        self._check_lens(lens, B)
        if dtype not in _DT:
            raise ValueError("resample: dtype must be torch.float32 or torch.int16")
        n_out = self.out_len(N)
        y = torch.empty(B, n_out, dtype=dtype, device=self.device) if out is None else out
        if y.dtype != dtype or tuple(y.shape) != (B, n_out) or y.device != self.device or (n_out > 1 and y.stride(1) != 1):
            raise ValueError(f"resample: out must be a {dtype} [{B}, {n_out}] tensor with unit sample stride")
        ol = torch.empty(B, dtype=torch.int32, device=self.device) if out_lens is None else out_lens
        self._check_lens(ol, B)
        self.launch(x, 0, N, 0, n_out, y, lens, lens_mul, ol)
        return y, ol

    def stream(self, B: int, lens=None, lens_mul=1, dtype=torch.float32, on_launch=None):
        """a chunked conversion of B rows: push(chunk [B, n], final=False) -> (first_out_sample, y_chunk); the
        concatenation of the pushes' chunks is the bits of the one-shot call on the concatenated input.  lens /
        lens_mul as __call__ (the rows' ends in absolute samples).  on_launch: called once per launch."""
        self._check_lens(lens, B)
        if dtype not in _DT:
            raise ValueError("resample: dtype must be torch.float32 or torch.int16")
        return ResampleStream(self, B, lens, lens_mul, dtype, on_launch)


class ResampleStream:
    """the state of one chunked conversion: the last K - 1 + M input samples, the absolute input position and the
    outputs emitted so far.  Every push is one launch of the one-shot kernel on (history | chunk) with the window's
    absolute position, over the output range span() gives."""

    def __init__(self, rs: Resampler, B, lens, lens_mul, dtype, on_launch):
        self.rs, self.B, self.lens, self.lens_mul, self.dtype, self.on_launch = rs, B, lens, lens_mul, dtype, on_launch
        self.keep = rs.K - 1 + rs.M
        self.hist = torch.empty(B, 0, dtype=torch.float32, device=rs.device)
        self.n_in = 0       # input samples pushed
        self.n_out = 0      # output samples emitted
        self.done = False

    def push(self, chunk, final=False):
        rs = self.rs
        if self.done:
            raise ValueError("resample stream: push after the final chunk")
        if chunk is None:
            chunk = self.hist[:, :0]
        rs._check_x(chunk)
        if chunk.shape[0] != self.B:
            raise ValueError(f"resample stream: chunk of {chunk.shape[0]} rows, stream of {self.B}")
        x = torch.cat([self.hist, chunk], 1) if self.hist.shape[1] else chunk
        x0 = self.n_in - self.hist.shape[1]
        self.n_in += chunk.shape[1]
        j0, j1 = span(self.n_in, final, self.n_out, rs.L, rs.M, rs.W)
        y = torch.empty(self.B, j1 - j0, dtype=self.dtype, device=rs.device)
        if j1 > j0:
            rs.launch(x, x0, self.n_in, j0, j1, y, self.lens, self.lens_mul)
            if self.on_launch is not None:
                self.on_launch()
        self.n_out = j1
        self.hist = x[:, max(0, x.shape[1] - self.keep):]
        if x is chunk:
            self.hist = self.hist.clone()  # (the caller's chunk may be a view of a buffer it rewrites)
        self.done = bool(final)
        return j0, y


_CACHE = {}


def resampler(device, sr_in: int, sr_out: int) -> Resampler:
    """the cached Resampler of (device, sr_in, sr_out); bad rates raise ValueError before anything is built"""
    ratio(sr_in, sr_out)
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (str(dev), int(sr_in), int(sr_out))
    rs = _CACHE.get(key)
    if rs is None:
        rs = _CACHE[key] = Resampler(dev, sr_in, sr_out)
    return rs
