"""Ragged frame batches through the prosody stage: predict_prosody(..., ragged_frames=True) on the
default engine, SPEC_TINY, B = 4 rows of T = 12 tokens -- with forced durations whose frame counts are [37, 9, 20, 2],
and with predicted durations on ragged text ([12, 5, 9, 3] tokens) at the same time.

Row b of the ragged batch must compute what the engine computes for that row alone at T40 = T_b: idx, en, the aligned
text rows, F0[b, :2 T_b] and N[b, :2 T_b] within max-abs <= 1e-6 of max|ref| (tests/test_gpu_scheduler.py's bound;
bit-identical is expected and which one it was is printed).  Tails as documented: idx -1, en and the aligned text rows
zero, F0 / N finite; frame_lens the rows' duration sums.  Rows of >= 3 frames are also held against the CPU oracle,
teacher-forced, at the bounds of tests/test_gpu_stages.py (F0 1e-4, N 3e-2, relative L2).  The same solo comparison on
a wider spec whose block convs take the register-direct form (T40 150, across the 128-row tile), with the F0 || N
fork on, and under graph capture with device durations and n_frames given (no host sync)."""
import pytest
import torch

from refops import rel_err

pytestmark = pytest.mark.gpu

B, T = 4, 12
FRAMES = [37, 9, 20, 2]
TEXT_LENS = [12, 5, 9, 3]


def _split(n, T=T):
    return [n // T + (1 if t < n % T else 0) for t in range(T)]


def _inputs(S, seed=99):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, T, S.d_txt, generator=g).to(torch.bfloat16).float()
    codes = torch.randn(B, S.L_s, S.code_dim, generator=g) * 0.3
    return h, codes


def _h_act(eng, h):
    from stzs.engine import Act
    t = torch.zeros(*h.shape, dtype=eng.adt, device=eng.device)
    t.copy_(h.to(eng.adt))
    return Act(t)


def _host(S, pro, ragged):
    """host copies of a predict_prosody result (the engine's buffers are reused by the next call)"""
    out = dict(idx=pro["idx"].cpu().clone(), en=pro["en"].t[:, :, :S.pr_in].float().cpu().clone(),
               asr=pro["asr_buf"].t[:, :, :S.d_txt].float().cpu().clone(), F0=pro["F0"].cpu().clone(),
               N=pro["N"].cpu().clone(), dur=pro["dur"].cpu().clone(), T40=pro["T40"])
    if ragged:
        out["frame_lens"] = pro["frame_lens"].cpu().clone()
    return out


def _near(tag, got, want):
    got, want = got.float(), want.float()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err = ((got - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()
    print(f"  {tag}: " + ("bit-identical" if torch.equal(got, want) else f"max-abs / max|ref| = {err:.2e}"))
    assert err <= 1e-6, (tag, err)


def _check_rows(rag, solos, frames):
    assert rag["frame_lens"].tolist() == frames and rag["T40"] == max(frames)
    for b, n in enumerate(frames):
        one = solos[b]
        print(f"row {b} ({n} frames)")
        assert one["T40"] == n
        assert torch.equal(rag["idx"][b, :n], one["idx"][0])
        _near("en", rag["en"][b, :n], one["en"][0])
        _near("aligned text", rag["asr"][b, :n], one["asr"][0])
        _near("F0", rag["F0"][b, :2 * n], one["F0"][0])
        _near("N", rag["N"][b, :2 * n], one["N"][0])
        assert bool((rag["idx"][b, n:] == -1).all())
        assert bool((rag["en"][b, n:] == 0).all()) and bool((rag["asr"][b, n:] == 0).all())
    assert bool(torch.isfinite(rag["F0"]).all()) and bool(torch.isfinite(rag["N"]).all())


@pytest.fixture(scope="module")
def eng(gpu_device, tiny, tiny_params):
    from stzs.engine import StyleTTSZS
    return StyleTTSZS(tiny, tiny_params, device=gpu_device)


_runs = {}


def _forced(eng, S):
    """the forced-durations ragged batch and every row's solo run, once"""
    if "forced" not in _runs:
        h, codes = _inputs(S)
        dur = torch.tensor([_split(n) for n in FRAMES], dtype=torch.int32)
        dev = eng.device
        rag = _host(S, eng.predict_prosody(_h_act(eng, h), codes.to(dev), dur, ragged_frames=True), True)
        solos = [_host(S, eng.predict_prosody(_h_act(eng, h[b:b + 1]), codes[b:b + 1].to(dev), dur[b:b + 1]), False)
                 for b in range(B)]
        assert eng.check_status() == 0
        _runs["forced"] = (h, codes, dur, rag, solos)
    return _runs["forced"]


def test_forced_durations_rows_match_solo(eng, tiny):
    _, _, dur, rag, solos = _forced(eng, tiny)
    _check_rows(rag, solos, FRAMES)
    assert torch.equal(rag["dur"], dur)


def test_rows_match_oracle(eng, tiny, tiny_params):
    """rows of >= 3 frames against the oracle run on the row alone, teacher-forced with the same text rows, codes and
    durations"""
    from oracle import stzs_ref as R
    h, codes, dur, rag, _ = _forced(eng, tiny)
    for b, n in enumerate(FRAMES):
        if n < 3:
            continue
        pr = R.predict_prosody(tiny_params, tiny, h[b:b + 1], codes[b:b + 1], dur[b:b + 1])
        assert torch.equal(rag["idx"][b:b + 1, :n], pr["idx"])
        eF, eN = rel_err(rag["F0"][b:b + 1, :2 * n], pr["F0"]), rel_err(rag["N"][b:b + 1, :2 * n], pr["N"])
        print(f"row {b} ({n} frames): F0 {eF:.2e} N {eN:.2e}")
        assert eF < 1e-4 and eN < 3e-2


def test_predicted_durations_with_ragged_text(eng, tiny):
    """predicted durations (one host sync sizes T40) on ragged text at the same time"""
    S, dev = tiny, eng.device
    h, codes = _inputs(S, 7)
    rag = _host(S, eng.predict_prosody(_h_act(eng, h), codes.to(dev), None, text_lens=TEXT_LENS, ragged_frames=True),
                True)
    frames = [int(rag["dur"][b, :n].sum()) for b, n in enumerate(TEXT_LENS)]
    assert bool((rag["dur"].sum(1) == torch.tensor(frames)).all())  # (the padding tokens take no frames)
    print("predicted frame counts", frames)
    solos = [_host(S, eng.predict_prosody(_h_act(eng, h[b:b + 1, :n]), codes[b:b + 1].to(dev)), False)
             for b, n in enumerate(TEXT_LENS)]
    assert eng.check_status() == 0
    _check_rows(rag, solos, frames)


def test_fork_rows_match_solo(gpu_device, tiny, tiny_params):
    """with the F0 || N fork on (side streams), the rows still equal the solo run"""
    from stzs.engine import StyleTTSZS
    S = tiny
    e2 = StyleTTSZS(S, tiny_params, device=gpu_device, branch_streams={"f0n"})
    h, codes = _inputs(S)
    dur = torch.tensor([_split(n) for n in FRAMES], dtype=torch.int32)
    rag = _host(S, e2.predict_prosody(_h_act(e2, h), codes.to(gpu_device), dur, ragged_frames=True), True)
    solos = [_host(S, e2.predict_prosody(_h_act(e2, h[b:b + 1]), codes[b:b + 1].to(gpu_device), dur[b:b + 1]), False)
             for b in range(B)]
    assert e2.check_status() == 0
    _check_rows(rag, solos, FRAMES)


def test_wider_spec_register_direct_rows_match_solo(gpu_device, tiny):
    """a spec whose predictor blocks take the register-direct conv form (128-channel inputs), T40 = 150 across the
    128-row tile edge"""
    from stzs import _lib as L
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    S = tiny.replace(d_txt=128, pr_hid=128, f0n_ch=(128, 128, 128))
    e2 = StyleTTSZS(S, init_params(S, seed=1), device=gpu_device)
    assert all(e2.W.pr_blk[f"pr.f0{i}"].conv1.frag32 and e2.W.pr_blk[f"pr.f0{i}"].conv2.frag32 for i in range(3))
    frames = [150, 9, 128, 2]
    h, codes = _inputs(S, 5)
    dur = torch.tensor([_split(n) for n in frames], dtype=torch.int32)
    rag = _host(S, e2.predict_prosody(_h_act(e2, h), codes.to(gpu_device), dur, ragged_frames=True), True)
    solos = [_host(S, e2.predict_prosody(_h_act(e2, h[b:b + 1]), codes[b:b + 1].to(gpu_device), dur[b:b + 1]), False)
             for b in range(B)]
    assert e2.check_status() == 0
    _check_rows(rag, solos, frames)


def test_device_only_path_captures(gpu_device, tiny, tiny_params):
    """device durations and n_frames given: no host sync, capturable; the replay equals the eager result"""
    from stzs.engine import StyleTTSZS
    S = tiny
    e2 = StyleTTSZS(S, tiny_params, device=gpu_device)  # (its own buffer cache: a capture pins its shapes)
    h, codes = _inputs(S)
    hd, cd = _h_act(e2, h), codes.to(gpu_device)
    dur = torch.tensor([_split(n) for n in FRAMES], dtype=torch.int32, device=gpu_device)

    def run():
        pro = e2.predict_prosody(hd, cd, dur, n_frames=max(FRAMES), ragged_frames=True)
        return pro["idx"], pro["en"].t, pro["asr_buf"].t, pro["F0"], pro["N"], pro["frame_lens"]

    eager = [t.clone() for t in run()]
    assert e2.check_status() == 0
    graph, outs = e2.capture(run)
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert graph.check() == 0
    for k, (a, b) in enumerate(zip(outs, eager)):
        assert torch.equal(a, b), k
    assert outs[5].tolist() == FRAMES


def test_row_helper_feeds_decode(eng, tiny):
    """prosody_rows: the rows of one frame count, cut out of a ragged result, decode to the solo run's waveform"""
    S, dev = tiny, eng.device
    h, codes = _inputs(S)
    frames = [20, 9, 20, 2]
    dur = torch.tensor([_split(n) for n in frames], dtype=torch.int32)
    pro = eng.predict_prosody(_h_act(eng, h), codes.to(dev), dur, ragged_frames=True)
    sub = eng.prosody_rows(pro, [0, 2], 20)
    wav = eng.decode(sub, codes[[0, 2]].to(dev), [5, 6]).clone()
    for j, b in enumerate((0, 2)):
        one = eng.predict_prosody(_h_act(eng, h[b:b + 1]), codes[b:b + 1].to(dev), dur[b:b + 1])
        w1 = eng.decode(one, codes[b:b + 1].to(dev), [5 + j])[0]
        err = ((wav[j] - w1).abs().max() / w1.abs().max()).item()
        print(f"row {b}:", "equal" if torch.equal(wav[j], w1) else f"max-rel {err:.2e}")
        assert err <= 1e-6
