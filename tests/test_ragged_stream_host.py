"""Ragged streaming, the host side (no GPU): the new keywords and their defaults, the two optional
trailing pointers of stzs_istft_stream_args in the ctypes mirror, the refusals of synth_stream(ragged_frames=True) and
of the ragged decode_chunked before any launch (the latency engine, the precise engines, the fp32 decoder, a spec whose
generator is on the generic conv path), the pure host schedule ragged_chunk_windows, the range check of host
frame_lens, and -- with the library built -- the alignment check of lens / post_off ahead of any runtime call."""
import ctypes as C
import inspect
import types

import pytest
import torch


def test_keywords_and_defaults():
    from stzs.engine import StyleTTSZS
    sig = lambda fn: inspect.signature(getattr(StyleTTSZS, fn)).parameters
    assert sig("synth_stream")["ragged_frames"].default is False
    assert sig("decode_chunked")["frame_lens"].default is None
    assert sig("istft_stream")["lens"].default is None
    # the uniform keywords keep their places and defaults
    assert sig("decode_chunked")["batch_windows"].default is True and sig("decode_chunked")["max_pass_rows"].default == 64
    assert sig("synth_stream")["chunked_halo"].default is None and sig("synth_stream")["chunk_s"].default == 1.0


def test_ctypes_fields():
    from stzs import _lib as L
    S = L.IstftStreamArgs
    assert [f[0] for f in S._fields_[-2:]] == ["lens", "post_off"]
    assert all(f[1] is L.opt_vp for f in S._fields_[-2:])
    assert S.lens.offset == S.hop_s.offset + 4 and S.post_off.offset == S.lens.offset + 8
    assert C.sizeof(S) == S.post_off.offset + 8 and C.sizeof(S) % 8 == 0
    a = S()
    assert not a.lens and not a.post_off  # NULL by default: the launch as before


def _engine_stub(**kw):
    """an engine object with just the attributes the ragged-decoder check reads: no device, no library"""
    from stzs.engine import StyleTTSZS
    e = StyleTTSZS.__new__(StyleTTSZS)
    e.blk_splitk, e.precise, e.precise_all, e.launches, e.dec_dt = 0, False, False, 0, torch.bfloat16
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _packed(spec):
    from stzs.params import init_params
    from stzs.weights import PackedModel
    return PackedModel(spec, init_params(spec, seed=0), torch.device("cpu"), fill=False)


@pytest.mark.parametrize("kw", [dict(blk_splitk=4), dict(precise=True, precise_all=True), dict(dec_dt=torch.float32),
                                dict(W="tiny")], ids=["latency", "precise", "fp32_decoder", "spec_tiny"])
def test_unsupported_engines_and_specs_raise_before_any_launch(kw, tiny):
    if kw.get("W") == "tiny":
        kw = dict(W=_packed(tiny))  # (SPEC_TINY: gen_ch 32 / 16, the generic conv_mfma path)
    e = _engine_stub(**kw)
    for call in (lambda: next(e.synth_stream(None, None, ragged_frames=True)),
                 lambda: next(e.synth_stream(None, None, ragged_frames=True, chunked_halo=1)),
                 lambda: next(e.decode_chunked(dict(T40=8), None, None, 2, 1, frame_lens=[8, 3]))):
        with pytest.raises(NotImplementedError):
            call()
    assert e.launches == 0


def test_ragged_chunk_windows():
    from stzs.engine import StyleTTSZS
    T, chunk, halo = [7, 1, 3, 6], 2, 1
    sched = StyleTTSZS.ragged_chunk_windows(T, chunk, halo)
    assert len(sched) == 4  # ceil(7 / 2)
    for k, rows in enumerate(sched):
        assert [b for b, _ in rows] == [b for b, n in enumerate(T) if chunk * k < n], k
    for b, n in enumerate(T):
        mine = [w for rows in sched for bb, w in rows if bb == b]
        assert mine == StyleTTSZS.chunk_windows(n, chunk, halo), b
    assert [w for bb, w in sched[2] if bb == 3] == [(4, 6, 2, 6)] and sched[3] == [(0, (6, 7, 3, 7))]
    # a uniform batch: every chunk holds every row on the uniform schedule
    uni = StyleTTSZS.ragged_chunk_windows([5, 5], 2, 1)
    assert [[w for _, w in rows] for rows in uni] == [[w, w] for w in StyleTTSZS.chunk_windows(5, 2, 1)]
    assert StyleTTSZS.ragged_chunk_windows([], 2, 1) == []


def test_check_frame_lens():
    from stzs.engine import check_frame_lens
    assert check_frame_lens([7, 1, 3, 6], 4, 7) == [7, 1, 3, 6]
    assert check_frame_lens(torch.tensor([7, 1], dtype=torch.int32), 2, 7) == [7, 1]
    for bad in ([0, 3], [8, 3], [3], [3, 3, 3], [2.0, 3.0], [[1, 2]], [True, True]):
        with pytest.raises(ValueError):
            check_frame_lens(bad, 2, 7)


@pytest.mark.parametrize("bad", [[0, 3], [9, 3], [3]], ids=["zero", "past_T40", "count"])
def test_out_of_range_frame_lens_raise_before_any_launch(bad, tiny):
    """on an engine that passes the ragged-decoder check: the host lengths are checked next, before anything runs"""
    e = _engine_stub(W=_packed(tiny.replace(dec_out=128, gen_ch=(256, 128))))
    pro = dict(T40=8, asr_buf=types.SimpleNamespace(B=2), F0=None, N=None)
    with pytest.raises(ValueError):
        next(e.decode_chunked(pro, None, None, 2, 1, frame_lens=bad))
    assert e.launches == 0


def _built():
    from stzs import _lib
    try:
        return _lib.load()
    except Exception:
        return None


def _ok_args(L):
    a = L.IstftStreamArgs()
    a.post, a.wav, a.tail_in, a.tail_out = 0x10000, 0x20000, 0x30000, 0x40000
    a.ldp, a.bsp, a.bsw, a.ldt = 24, 24 * 64, 4096, 24
    a.B, a.f0, a.Fc, a.final_chunk, a.n_fft, a.hop_s = 2, 8, 8, 0, 20, 5
    return a


def test_misaligned_lens_and_post_off_are_refused_without_a_runtime_call():
    """the pointers are never dereferenced and no stream exists: anything but an early return would crash or fail
    differently.  The same arguments with empty shapes reach the shape checks (STZS_ESHAPE): EINVAL is the alignment."""
    from stzs import _lib as L
    lib = _built()
    assert lib is not None, "the library is not built (styletts-zs_amd/build.py)"
    for field in ("lens", "post_off"):
        for off in (1, 2, 3):
            a = _ok_args(L)
            setattr(a, field, 0x50000 + off)
            assert lib.stzs_istft_stream(C.byref(a), None) == L.EINVAL, (field, off)
        a = _ok_args(L)
        setattr(a, field, 0x50004)  # aligned: past the pointer checks, refused for its shape alone
        a.B = 0
        assert lib.stzs_istft_stream(C.byref(a), None) == L.ESHAPE, field
