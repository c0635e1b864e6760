"""Ragged text batches, the host side (no GPU): the scheduler's phase-1 grouping with and without ragged_text, the
range check of host-side text_lens, and the text_lens keyword on the public entry points."""
import inspect

import pytest
import torch


def _reqs():
    """the request mix of tests/test_gpu_scheduler.py (token count, reference length, forced durations)"""
    from stzs.scheduler import Request
    from stzs.spec import SPEC_TINY as S
    g = torch.Generator().manual_seed(21)
    reqs = []
    for k, (T, nref, forced) in enumerate([(8, S.sr, None), (12, S.sr, None), (12, S.sr, None),
                                           (8, S.sr + S.sr // 2, None), (10, S.sr, [4] * 10), (8, S.sr, [5] * 8),
                                           (6, S.sr, None)]):
        reqs.append(Request(tokens=torch.randint(1, S.n_symbols, (T,), generator=g),
                            ref_wav=torch.randn(nref, generator=g) * 0.1,
                            noise=torch.randn(S.L_s, S.code_dim, generator=g), seed=100 + k,
                            durations=torch.tensor(forced, dtype=torch.int32) if forced else None))
    return reqs


def test_phase1_groups_both_settings():
    from stzs.scheduler import BucketScheduler
    reqs = _reqs()
    plain = BucketScheduler(None, max_batch=4).phase1_groups(reqs)
    assert plain == [(False, [0]), (False, [1, 2]), (False, [3]), (True, [4]), (True, [5]), (False, [6])]
    ragged = BucketScheduler(None, max_batch=4, ragged_text=True).phase1_groups(reqs)
    # by (reference length, forced) only: the four 1-s unforced requests of 8 / 12 / 12 / 6 tokens share a batch
    assert ragged == [(False, [0, 1, 2, 6]), (False, [3]), (True, [4, 5])]
    # chunks of at most max_batch, in request order; every request exactly once
    small = BucketScheduler(None, max_batch=3, ragged_text=True).phase1_groups(reqs)
    assert small == [(False, [0, 1, 2]), (False, [6]), (False, [3]), (True, [4, 5])]
    for groups in (plain, ragged, small):
        assert sorted(i for _, ch in groups for i in ch) == list(range(len(reqs)))
    assert BucketScheduler(None).ragged_text is False  # off by default


def test_host_text_lens_range_check():
    from stzs.engine import check_text_lens
    ok = check_text_lens([12, 5, 9, 3], 4, 12)
    assert ok.dtype == torch.int32 and ok.tolist() == [12, 5, 9, 3]
    assert check_text_lens(torch.tensor([1, 12]), 2, 12).tolist() == [1, 12]
    for bad in ([0, 5, 9, 3], [13, 5, 9, 3], [-1, 5, 9, 3]):  # 0, T + 1, negative
        with pytest.raises(ValueError):
            check_text_lens(bad, 4, 12)
    for bad in ([12, 5, 9], [[12, 5, 9, 3]], 7, [1.0, 2.0, 3.0, 4.0]):  # wrong shape / not integers
        with pytest.raises(ValueError):
            check_text_lens(bad, 4, 12)


def test_text_lens_keyword_on_the_public_entry_points():
    from stzs.engine import StyleTTSZS
    from stzs.scheduler import BucketScheduler
    for fn in ("text_encode", "sample_style", "denoiser_prepare", "duration_encoder", "predict_durations",
               "predict_prosody", "_front", "synth", "synth_stream"):
        p = inspect.signature(getattr(StyleTTSZS, fn)).parameters
        assert "text_lens" in p and p["text_lens"].default is None, fn
    assert inspect.signature(BucketScheduler.__init__).parameters["ragged_text"].default is False


def test_abi_has_the_length_fields():
    """the ctypes mirror carries every new optional pointer (tests/test_abi.py compares the layouts with the header)"""
    from stzs import _lib as L
    for struct, field in ((L.RowLNArgs, "lens"), (L.RowLNArgs, "T"), (L.AttnArgs, "lk_rows"), (L.LstmArgs, "lens"),
                          (L.PrPrepArgs, "lens"), (L.DurArgs, "lens"), (L.CopyArgs, "dst_row_off")):
        assert field in [f for f, _ in struct._fields_], (struct.__name__, field)
    assert "stzs_embed_lens" in L.EXPORTS
    p = 0x1000
    lib = L.load()
    assert lib.stzs_embed_lens(p, p, p, None, 1, 1, 8, 8, L.BF16, None) == L.EINVAL  # lens is required here
    assert lib.stzs_embed_lens(p, p, p, p, 1, 0, 8, 8, L.BF16, None) == L.ESHAPE
    a = L.RowLNArgs()
    a.x, a.y, a.lens = p, p, p
    a.R, a.C, a.gdiv, a.ldx, a.ldy, a.T = 12, 64, 1, 64, 64, 5
    assert lib.stzs_row_layernorm(a, None) == L.ESHAPE  # R is not a whole number of T-row blocks
