"""Ragged reference batches, the host side (no GPU): the scheduler's phase-1 grouping under the four
(ragged_text, ragged_ref) settings, the range check of host-side ref_lens, the ref_lens keyword on the public entry
points, the new ctypes fields / the stzs_mask_rows export, and the library's error codes on placeholder pointers
(every check runs before any HIP call: nothing is dereferenced)."""
import ctypes as C
import inspect

import pytest
import torch


def _reqs():
    """the request mix of tests/test_gpu_scheduler.py with three reference lengths (1 s, 1.5 s, 0.75 s)"""
    from stzs.scheduler import Request
    from stzs.spec import SPEC_TINY as S
    g = torch.Generator().manual_seed(21)
    reqs = []
    for k, (T, nref, forced) in enumerate([(8, S.sr, None), (12, S.sr, None), (12, 3 * S.sr // 4, None),
                                           (8, S.sr + S.sr // 2, None), (10, S.sr, [4] * 10),
                                           (8, 3 * S.sr // 4, [5] * 8), (6, S.sr, None)]):
        reqs.append(Request(tokens=torch.randint(1, S.n_symbols, (T,), generator=g),
                            ref_wav=torch.randn(nref, generator=g) * 0.1,
                            noise=torch.randn(S.L_s, S.code_dim, generator=g), seed=100 + k,
                            durations=torch.tensor(forced, dtype=torch.int32) if forced else None))
    return reqs


def test_phase1_groups_four_settings():
    from stzs.scheduler import BucketScheduler
    reqs = _reqs()

    def groups(**kw):
        return BucketScheduler(None, max_batch=4, **kw).phase1_groups(reqs)
    plain = groups()
    assert plain == [(False, [0]), (False, [1]), (False, [2]), (False, [3]), (True, [4]), (True, [5]), (False, [6])]
    text = groups(ragged_text=True)  # by (reference length, forced)
    assert text == [(False, [0, 1, 6]), (False, [2]), (False, [3]), (True, [4]), (True, [5])]
    ref = groups(ragged_ref=True)  # by (token count, forced)
    assert ref == [(False, [0, 3]), (False, [1, 2]), (True, [4]), (True, [5]), (False, [6])]
    both = groups(ragged_text=True, ragged_ref=True)  # by (forced,) alone
    assert both == [(False, [0, 1, 2, 3]), (False, [6]), (True, [4, 5])]
    small = BucketScheduler(None, max_batch=2, ragged_text=True, ragged_ref=True).phase1_groups(reqs)
    assert small == [(False, [0, 1]), (False, [2, 3]), (False, [6]), (True, [4, 5])]
    for g, mb in ((plain, 4), (text, 4), (ref, 4), (both, 4), (small, 2)):
        assert sorted(i for _, ch in g for i in ch) == list(range(len(reqs)))  # every request exactly once
        assert all(1 <= len(ch) <= mb for _, ch in g)
    sch = BucketScheduler(None)
    assert sch.ragged_text is False and sch.ragged_ref is False  # both off by default


def test_host_ref_lens_range_check():
    from stzs.engine import check_ref_lens
    from stzs.spec import SPEC_TINY as S
    lo, N = S.mel_nfft // 2 + 1, 4500
    ok = check_ref_lens([N, lo, 2999, 3000], 4, N, S.mel_nfft)
    assert ok.dtype == torch.int32 and ok.tolist() == [N, lo, 2999, 3000]
    assert check_ref_lens(torch.tensor([lo, N]), 2, N, S.mel_nfft).tolist() == [lo, N]
    for bad in ([lo - 1, N, N, N], [N + 1, N, N, N], [-1, N, N, N], [0, N, N, N]):
        with pytest.raises(ValueError):
            check_ref_lens(bad, 4, N, S.mel_nfft)
    for bad in ([N, N, N], [[N, N, N, N]], N, [float(N)] * 4, [True] * 4):  # wrong shape / not integers
        with pytest.raises(ValueError):
            check_ref_lens(bad, 4, N, S.mel_nfft)


def test_ref_lens_keyword_on_the_public_entry_points():
    from stzs.engine import StyleTTSZS
    from stzs.scheduler import BucketScheduler
    for fn in ("log_mel", "prompt_features", "prompt_encode", "encode_inputs", "_front", "synth", "synth_stream"):
        p = inspect.signature(getattr(StyleTTSZS, fn)).parameters
        assert "ref_lens" in p and p["ref_lens"].default is None, fn
    assert inspect.signature(BucketScheduler.__init__).parameters["ragged_ref"].default is False


def test_abi_has_the_reference_length_fields():
    """the ctypes mirror carries every new optional pointer (tests/test_abi.py and tests/test_precise_frontend_host.py
    compare the layouts with the header) and the library answers bad calls with codes before any launch"""
    from stzs import _lib as L
    for struct, field in ((L.FramesArgs, "n_lens"), (L.FramesArgs, "f_lens_out"), (L.StftMelArgs, "n_lens"),
                          (L.StftMelArgs, "f_lens_out"), (L.LogMelArgs, "lens"), (L.PoolArgs, "lens"),
                          (L.MaskArgs, "lens")):
        assert field in [f for f, _ in struct._fields_], (struct.__name__, field)
        assert C.sizeof(dict(struct._fields_)[field]) == C.sizeof(C.c_void_p)
    assert "stzs_mask_rows" in L.EXPORTS
    lib = L.load()
    p = 0x1000
    # stzs_mask_rows: NULL args / x / lens -> EINVAL, shapes -> ESHAPE, dtype -> EDTYPE
    assert lib.stzs_mask_rows(None, None) == L.EINVAL

    def mask(**kw):
        a = L.MaskArgs()
        a.x, a.lens, a.ld, a.bs, a.B, a.T, a.C, a.dtype = p, p, 32, 16 * 32, 4, 16, 32, L.BF16
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.stzs_mask_rows(C.byref(a), None)
    assert mask(lens=None) == L.EINVAL and mask(x=None) == L.EINVAL
    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(C=0), dict(ld=31), dict(bs=15 * 32 + 31), dict(T=-1)):
        assert mask(**kw) == L.ESHAPE, kw
    assert mask(dtype=L.I32) == L.EDTYPE and mask(dtype=L.F8) == L.EDTYPE
    # f_lens_out is the ragged launch's output: without n_lens -> EINVAL (both STFT entry points); with both set the
    # shape checks still come first
    f = L.FramesArgs()
    f.wav, f.window, f.y, f.f_lens_out = p, p, p, p
    f.ldw, f.ldy, f.bsy, f.B, f.N, f.F, f.n_fft, f.win, f.hop = 4500, 1200, 16 * 1200, 4, 4500, 16, 2048, 1200, 300
    assert lib.stzs_stft_frames(C.byref(f), None) == L.EINVAL
    f.n_lens, f.N = p, 1024  # reflect padding needs N > n_fft / 2
    assert lib.stzs_stft_frames(C.byref(f), None) == L.ESHAPE
    s = L.StftMelArgs()
    for fld, ct in L.StftMelArgs._fields_:
        if ct is C.c_void_p:
            setattr(s, fld, p)
    s.ldw, s.ldy, s.bsy = 4500, 16, 16 * 16
    s.B, s.N, s.F, s.n_fft, s.win, s.hop, s.n_mels, s.out_dtype = 4, 4500, 16, 2048, 1200, 300, 16, L.F32
    s.f_lens_out = p
    assert lib.stzs_stft_logmel(C.byref(s), None) == L.EINVAL
    s.n_lens, s.N = p, 1024
    assert lib.stzs_stft_logmel(C.byref(s), None) == L.ESHAPE
    # lens on the log-mel and the pool: optional, the shape checks unchanged
    m = L.LogMelArgs()
    m.spec, m.fb, m.ranges, m.y, m.lens = p, p, p, p, p
    assert lib.stzs_log_mel(C.byref(m), None) == L.ESHAPE
    q = L.PoolArgs()
    q.x, q.y, q.lens = p, p, p
    assert lib.stzs_pool_rows(C.byref(q), None) == L.ESHAPE
