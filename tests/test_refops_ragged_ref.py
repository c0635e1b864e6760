"""The padded-batch algorithm of a ragged reference batch, emulated in torch on the CPU with the
oracle's own log_mel / _conv / _lin and held against oracle prompt_features of every row alone at its own length.

The emulation is the engine's sequence: each row's own log-mel (its own reflection, its own F_b = n // hop + 1 frames)
in a padded block whose rows t >= F_b are zero; pe.conv0 + LeakyReLU over the block; the tail rows of its output
(LeakyReLU(bias)) zeroed; pe.conv1 + LeakyReLU; adaptive pooling over [0, F_b) per row; pe.proj.

Bound: 1.8e-6 max-abs over max|ref|, 4x the larger figure measured for this emulation on these two batches (4.3e-7,
3.1e-7): fp32 rounding of two summation groupings of the same convolution (a padded block against a short one), not
a property of the code under test.  Each of three planted defects -- no mask on c0, pooling over the padded frame
count, reflection at the padded N -- must leave that bound, or the test would not see the defect in the kernels."""
import pytest
import torch
import torch.nn.functional as F

BATCHES = {"short": (4500, [4500, 1025, 2999, 3000]), "tile": (39000, [39000, 38400, 38399, 1025])}
BOUND = 1.8e-6


def _wav(N, B=4):
    return torch.randn(B, N, generator=torch.Generator().manual_seed(N)) * 0.1


def padded_batch(P, S, wav, lens, mask_c0=True, pool_own=True, reflect_own=True):
    from oracle import stzs_ref as R
    B, N = wav.shape
    Fr = N // S.hop + 1
    fb = [n // S.hop + 1 for n in lens]
    mel = torch.zeros(B, S.n_mels, Fr)
    for b, n in enumerate(lens):
        if reflect_own:
            mel[b, :, :fb[b]] = R.log_mel(wav[b:b + 1, :n], S)[0]
        else:  # the planted defect: frames of the padded row (reflection at N, samples past n read as the zero padding)
            full = torch.cat([wav[b, :n], torch.zeros(N - n)])[None]
            mel[b, :, :fb[b]] = R.log_mel(full, S)[0, :, :fb[b]]
    keep = (torch.arange(Fr)[None] < torch.tensor(fb)[:, None])[:, None].float()  # [B, 1, Fr]
    x = F.leaky_relu(R._conv(mel, P, "pe.conv0", padding=2), 0.2)
    if mask_c0:
        x = x * keep
    x = F.leaky_relu(R._conv(x, P, "pe.conv1", padding=2), 0.2)
    rows = []
    for b in range(B):
        T = fb[b] if pool_own else Fr
        rows.append(F.adaptive_avg_pool1d(x[b:b + 1, :, :T], S.L_s).transpose(1, 2))
    return R._lin(torch.cat(rows), P, "pe.proj")


_solo = {}


def _solo_rows(P, S, name):
    """oracle prompt_features of each row alone on its own samples: computed once per batch, shared"""
    if name not in _solo:
        from oracle import stzs_ref as R
        N, lens = BATCHES[name]
        wav = _wav(N)
        _solo[name] = [R.prompt_features(P, S, wav[b:b + 1, :n])[0] for b, n in enumerate(lens)]
    return _solo[name]


def _errs(got, solo):
    return [((got[b] - w).abs().max() / w.abs().max()).item() for b, w in enumerate(solo)]


@pytest.mark.parametrize("name", list(BATCHES))
def test_padded_batch_equals_rows_alone(tiny, tiny_params, name):
    N, lens = BATCHES[name]
    errs = _errs(padded_batch(tiny_params, tiny, _wav(N), lens), _solo_rows(tiny_params, tiny, name))
    print(name, "max-abs / max|ref| per row", ["%.1e" % e for e in errs])
    assert max(errs) <= BOUND


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("defect", ["mask_c0", "pool_own", "reflect_own"])
def test_planted_defects_leave_the_bound(tiny, tiny_params, name, defect):
    N, lens = BATCHES[name]
    errs = _errs(padded_batch(tiny_params, tiny, _wav(N), lens, **{defect: False}), _solo_rows(tiny_params, tiny, name))
    print(name, "without", defect, ["%.1e" % e for e in errs])
    # the full-length row has no tail: it stays inside; every shorter row must leave
    assert errs[0] <= BOUND
    assert min(errs[1:]) > BOUND
