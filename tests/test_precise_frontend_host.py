"""The precise reference-prompt front end, host side (no GPU): the stzs_stft_logmel entry point validates its
arguments before any HIP call, its ctypes struct matches the C layout, the packed FFT twiddle table is the float64
cos | -sin rounded once, and PackedModel(precise_frontend=True) packs the split streams of the prompt encoder."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import torch

from conftest import ROOT


def _args(L_):
    """a shape-valid call (v0's front end on a 1-s wav) with placeholder pointers: nothing is dereferenced by the checks"""
    a = L_.StftMelArgs()
    for f, ct in L_.StftMelArgs._fields_:
        if ct is C.c_void_p:
            setattr(a, f, 0x1000)
    a.B, a.N, a.F, a.n_fft, a.win, a.hop, a.n_mels, a.out_dtype = 2, 24000, 81, 2048, 1200, 300, 80, L_.F32
    a.ldw, a.ldy, a.bsy = 24000, 80, 81 * 80
    return a


def test_stft_logmel_rejects_before_launch():
    from stzs import _lib
    L = _lib.load()
    fn = L.stzs_stft_logmel
    assert fn(None, None) == _lib.EINVAL
    a = _lib.StftMelArgs()  # all zero: required pointers NULL
    assert fn(C.byref(a), None) == _lib.EINVAL
    for f, ct in _lib.StftMelArgs._fields_:
        if ct is C.c_void_p:
            setattr(a, f, 0x1000)
    assert fn(C.byref(a), None) == _lib.ESHAPE  # sizes all 0
    for f, _ct in _lib.StftMelArgs._fields_:  # each required pointer on its own
        if _ct is C.c_void_p:
            a = _args(_lib)
            setattr(a, f, None)
            assert fn(C.byref(a), None) == _lib.EINVAL, f
    bad = [dict(n_fft=1000), dict(N=1024),  # not a power of two; N = n_fft / 2: no reflect padding
           dict(n_fft=32, win=32), dict(n_fft=8192), dict(win=2049), dict(F=(24000 + 2048) // 300 + 2), dict(ldy=79),
           dict(ldw=23999), dict(B=0), dict(B=-1), dict(F=0), dict(hop=0), dict(win=0), dict(n_mels=0), dict(N=-5)]
    for kw in bad:
        a = _args(_lib)
        for k, v in kw.items():
            setattr(a, k, v)
        assert fn(C.byref(a), None) == _lib.ESHAPE, kw
    a = _args(_lib)
    a.out_dtype = _lib.I32
    assert fn(C.byref(a), None) == _lib.EDTYPE


def test_stftmel_struct_matches_c_layout():
    """gcc probe against include/stzs.h: sizeof and every field offset of stzs_stftmel_args."""
    from stzs import _lib
    py = _lib.StftMelArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stzs.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(stzs_stftmel_args));']
    for f, _t in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(stzs_stftmel_args, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = subprocess.run([exe], capture_output=True, text=True).stdout.split()
    got = dict(zip(out[0::2], (int(v) for v in out[1::2])))
    assert got["size"] == C.sizeof(py)
    for f, _t in py._fields_:
        assert got[f] == getattr(py, f).offset, f
    assert len(got) == len(py._fields_) + 1


def test_twiddle_table_is_float64_rounded_once(tiny, tiny_params):
    from stzs.weights import PackedModel, stft_twiddles
    W = PackedModel(tiny, tiny_params, device="cpu", precise_frontend=True)
    tw = W.t(W.fe_tw)
    n = tiny.mel_nfft
    assert tw.dtype == torch.float32 and tuple(tw.shape) == (n, 2)
    want = torch.tensor([[math.cos(2.0 * math.pi * q / n), -math.sin(2.0 * math.pi * q / n)] for q in range(n)],
                        dtype=torch.float64).float()
    assert torch.equal(tw, want)
    assert torch.equal(stft_twiddles(64), want[::n // 64])  # (exact angles: the coarser table is a subset)


def test_packed_model_split_streams(tiny, tiny_params):
    from stzs.weights import PackedModel
    on = PackedModel(tiny, tiny_params, device="cpu", precise_frontend=True)
    off = PackedModel(tiny, tiny_params, device="cpu")
    assert on.precise_frontend and not off.precise_frontend
    for nm in ("pe_conv0", "pe_conv1", "pe_proj"):
        assert getattr(on, nm).wx3 is not None, nm
        assert getattr(off, nm).wx3 is None and getattr(off, nm).fx3 is None, nm
    assert off.fe_tw is None and off.fe_dft is not None
    assert on.fe_dft is None and "fe.dft.wpk" not in on.arena.views  # the bf16 DFT basis is not carried
    assert on.arena.buf.numel() < off.arena.buf.numel()
    # the flag touches the front end only
    assert on.te_conv[0].wx3 is None and not on.precise and not on.precise_all
