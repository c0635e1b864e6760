"""Enrolled voices without a device: the C layout of stzs_voice_args, every rejection of
stzs_voice_prompt before a launch, the host checks of VoiceRows / enroll / VoiceBank (engines on "cpu" over the recording
stand-in of tools/launch_trace.py: nothing is launched), the scheduler's phase-1 grouping of voice requests, and the
properties of the numpy reference that make the GPU cases exact."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

from refops_voice import mix_ref  # noqa: E402


# ------------------------------------------------------------------ ABI
def test_voice_args_match_c_layout():
    """sizeof and every field offset of stzs_voice_args, compiled with gcc from the header, against VoiceArgs"""
    from stzs import _lib
    py = _lib.VoiceArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stzs.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(stzs_voice_args));']
    for f, _t in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(stzs_voice_args, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = dict((a, int(b)) for a, b in (ln.split() for ln in
                                            subprocess.run([exe], capture_output=True, text=True).stdout.split("\n") if ln))
    assert got["size"] == C.sizeof(py)
    for f, _t in py._fields_:
        assert got[f] == getattr(py, f).offset, f
    assert "stzs_voice_prompt" in _lib.EXPORTS


def _ok_args():
    """arguments stzs_voice_prompt would launch with (fake, aligned pointers): every case below breaks one thing"""
    from stzs import _lib
    a = _lib.VoiceArgs()
    a.zbank, a.ibank, a.codebook, a.src, a.w, a.cnt = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    a.idx, a.y, a.zmix = 0x70000, 0x80000, 0x90000
    a.ldz, a.ldib, a.ldi, a.ldy, a.ldm = 64, 8, 8, 64, 64
    a.V, a.L, a.B, a.Kmax, a.G, a.K, a.dg, a.gather = 3, 8, 2, 2, 8, 256, 8, 0
    return a


def test_voice_prompt_rejects_before_launch():
    """every rejection the header lists returns its code; nothing is launched (no device exists here: a launch would
    not return a validation code)"""
    from stzs import _lib
    # (the library itself, whatever stands in for stzs._lib.load while the `host` fixture of this module is alive)
    fn = C.CDLL(_lib.LIB_PATH).stzs_voice_prompt
    fn.argtypes, fn.restype = [C.POINTER(_lib.VoiceArgs), C.c_void_p], C.c_int32
    E, S = _lib.EINVAL, _lib.ESHAPE
    assert fn(None, None) == E
    assert fn(C.byref(_lib.VoiceArgs()), None) == E
    for f in ("zbank", "codebook", "src", "w", "cnt", "idx", "y"):
        a = _ok_args()
        setattr(a, f, None)
        assert fn(C.byref(a), None) == E, f
    a = _ok_args()
    a.gather, a.ibank = 1, None
    assert fn(C.byref(a), None) == E  # gather without ibank
    for f in ("zbank", "ibank", "codebook", "src", "w", "cnt", "idx", "y", "zmix"):
        a = _ok_args()
        v = getattr(a, f)
        setattr(a, f, (v if isinstance(v, int) else v.value) + 2)
        assert fn(C.byref(a), None) == E, f  # not 4-byte aligned
    for f in ("V", "L", "B", "Kmax", "G", "K"):
        for v in (0, -1):
            a = _ok_args()
            setattr(a, f, v)
            assert fn(C.byref(a), None) == S, (f, v)
    a = _ok_args()
    a.Kmax = 9
    assert fn(C.byref(a), None) == S
    for dg in (0, 2, 3, 12, 32):
        a = _ok_args()
        a.dg = dg
        assert fn(C.byref(a), None) == S, dg
    a = _ok_args()
    a.K = (64 * 1024 - 2048) // (8 * 4) + 1  # one entry past 64 KB of LDS with the scan's 2 KB of partials
    assert fn(C.byref(a), None) == S
    for f, v in (("ldz", 63), ("ldi", 7), ("ldy", 63), ("ldm", 63)):
        a = _ok_args()
        setattr(a, f, v)
        assert fn(C.byref(a), None) == S, f
    a = _ok_args()
    a.gather, a.ldib = 1, 7
    assert fn(C.byref(a), None) == S
    a = _ok_args()  # every pointer set, all sizes zero: rejected, nothing dereferenced (the rule of tests/test_abi.py)
    a.V = a.L = a.B = a.Kmax = a.G = a.K = a.dg = 0
    assert fn(C.byref(a), None) == S


# ------------------------------------------------------------------ weights, rows, enroll, bank
def test_weight_normalisation():
    from stzs.voice import normalise_weights
    for one in (1.0, 0.3, 7, 1e-30, 3e30):
        assert normalise_weights([one], 1) == [1.0]  # exactly 1.0 for one source
    assert normalise_weights(None, 1) == [1.0]
    assert normalise_weights(None, 4) == [0.25] * 4
    assert normalise_weights([1, 1, 2], 3) == [0.25, 0.25, 0.5]
    w = normalise_weights([0.3, 0.7], 2)
    assert w == [float(np.float32(0.3 / 1.0)), float(np.float32(0.7 / 1.0))]
    w = normalise_weights([1, 1, 1], 3)
    assert w == [float(np.float32(1.0 / 3.0))] * 3  # the division in float64, rounded once
    for bad in ([float("nan"), 1.0], [float("inf"), 1.0], [-0.5, 1.5], [0.0, 0.0], [1.0], [1.0, 2.0, 3.0], ["a", 1]):
        with pytest.raises(ValueError):
            normalise_weights(bad, 2)


@pytest.fixture(scope="module")
def host(tiny, tiny_params):
    """two engines on "cpu" over the recording library (different prompt encoders), and the recorder"""
    import launch_trace as LT
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    with LT._Patched() as lib:
        eng = StyleTTSZS(tiny, tiny_params, device="cpu")
        other = StyleTTSZS(tiny, init_params(tiny, seed=1), device="cpu")
        yield eng, other, lib


def _voice(eng, seed):
    from stzs.voice import Voice
    S = eng.spec
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(S.L_s, S.code_dim, generator=g)
    idx = torch.randint(0, S.vq_size, (S.L_s, S.code_dim // S.vq_group), generator=g).to(torch.int32)
    return Voice(z, idx, eng.voice_fingerprint(), clips=1 + seed % 3, frontend="bf16")


def test_voice_rows_checks_and_structure(host):
    from stzs.voice import VoiceBank
    eng, _, lib = host
    bank = VoiceBank(eng, 4)
    for s in range(3):
        assert bank.add(_voice(eng, s)) == s
    n = len(lib.calls)
    rows = eng.voice_rows(3, bank, [2, 0, 1])
    assert rows.gather and rows.Kmax == 1 and rows.src.tolist() == [[2], [0], [1]] and rows.w.tolist() == [[1.0]] * 3
    assert rows.cnt.tolist() == [1, 1, 1] and rows.src.dtype == torch.int32 and rows.w.dtype == torch.float32
    assert eng.voice_rows(3, bank, torch.tensor([2, 0, 1])).src.tolist() == [[2], [0], [1]]
    mix = eng.voice_rows(3, bank, [[0, 1], [2], [0, 1, 2]], [[0.3, 0.7], None, [1, 1, 2]])
    assert not mix.gather and mix.Kmax == 3 and mix.cnt.tolist() == [2, 1, 3]
    assert mix.w[0, :2].tolist() == [float(np.float32(0.3)), float(np.float32(0.7))] and mix.w[1, 0].item() == 1.0
    assert mix.w[2].tolist() == [0.25, 0.25, 0.5] and mix.src[2].tolist() == [0, 1, 2]
    for ids, w in (([0, 1], None), ([0, 1, 3], None), ([0, 1, -1], None), ([0, 1, 1.5], None), ([0, 1, True], None),
                   ([[0, 1], [2], []], None), ([[0] * 9, [1], [2]], None), ([[0, 1], [2], [0]], [[1, 1], [1]]),
                   ([[0, 1], [2], [0]], [[1, -1], [1], [1]]), ([[0, 1], [2], [0]], [[0, 0], [1], [1]]),
                   ([[0, 1], [2], [0]], [[1, float("nan")], [1], [1]]), ([[0, 1], [2], [0]], [[1], [1], [1]])):
        with pytest.raises(ValueError):
            eng.voice_rows(3, bank, ids, w)
    with pytest.raises(ValueError):
        eng.voice_rows(0, bank, [])
    # set(): values in place, structure refused with nothing written
    p = (rows.src.data_ptr(), rows.w.data_ptr(), rows.cnt.data_ptr())
    rows.set([1, 1, 0])
    assert rows.src.tolist() == [[1], [1], [0]] and p == (rows.src.data_ptr(), rows.w.data_ptr(), rows.cnt.data_ptr())
    with pytest.raises(ValueError):
        rows.set([[0, 1], 1, 0])  # a blend in the gather form
    with pytest.raises(ValueError):
        rows.set([1, 3, 0])
    assert rows.src.tolist() == [[1], [1], [0]]
    before = (mix.src.clone(), mix.w.clone(), mix.cnt.clone())
    with pytest.raises(ValueError):
        mix.set([[0, 1, 2, 0], [2], [0]])  # more sources than Kmax
    with pytest.raises(ValueError):
        mix.set([[0, 1], [2]])
    assert all(torch.equal(a, b) for a, b in zip(before, (mix.src, mix.w, mix.cnt)))
    mix.set([[2], [1, 0], [0, 0, 1]], [None, [3, 1], None])  # (single-voice rows are fine in the mix form: cnt 1)
    assert mix.cnt.tolist() == [1, 2, 3] and mix.w[1, :2].tolist() == [0.75, 0.25] and not mix.gather
    with pytest.raises(ValueError):
        rows.rows(2)
    assert len(lib.calls) == n  # none of this launched anything


def test_enroll_and_synth_argument_checks(host, tiny):
    from stzs.voice import VoiceBank
    eng, _, lib = host
    S = tiny
    n, launches = len(lib.calls), eng.launches
    clip = torch.randn(3, 3000) * 0.1
    for kw in (dict(ref_wav=torch.randn(9, 3000)), dict(ref_wav=torch.randn(2, 2, 3000)),
               dict(ref_wav=clip, weights=[1, 1]), dict(ref_wav=clip, weights=[1, -1, 1]),
               dict(ref_wav=clip, weights=[0, 0, 0]), dict(ref_wav=clip, weights=[1, float("inf"), 1]),
               dict(ref_wav=clip, weights=[1, float("nan"), 1]), dict(ref_wav=torch.zeros(3000, dtype=torch.int32))):
        with pytest.raises(ValueError):
            eng.enroll(**kw)
    bank = VoiceBank(eng, 2)
    bank.add(_voice(eng, 0))
    rows = eng.voice_rows(2, bank, [0, 0])
    tok = torch.ones(2, 4, dtype=torch.int32)
    eps = torch.zeros(2, S.L_s, S.code_dim)
    G = S.code_dim // S.vq_group
    for ref, kw in ((clip[:2], {}), (None, dict(prompt_idx=torch.zeros(2, S.L_s, G, dtype=torch.int32))),
                    (None, dict(ref_lens=[3000, 3000])), (None, dict(ref_sr=16000))):
        with pytest.raises(ValueError):
            eng.synth(tok, ref, noise=eps, voices=rows, **kw)
        with pytest.raises(ValueError):
            next(eng.synth_stream(tok, ref, noise=eps, voices=rows, **kw))
    with pytest.raises(ValueError):
        eng.encode_inputs(tok, clip[:2], voices=rows)
    with pytest.raises(ValueError):
        eng.synth(tok[:1], None, noise=eps[:1], voices=rows)  # rows made for another batch size
    with pytest.raises(ValueError):
        eng.synth(tok, None, noise=eps, voices=object())
    assert len(lib.calls) == n and eng.launches == launches


def test_one_launch_prompt_in_the_trace(host, tiny):
    """host trace (recording library): synth(voices=) makes the calls of synth(ref_wav=) with ONE stzs_voice_prompt
    where the front end's calls stood -- and a call without voices makes the calls it made before"""
    from stzs.voice import VoiceBank
    eng, _, lib = host
    S = tiny
    g = torch.Generator().manual_seed(5)
    B, T = 2, 6
    tok = torch.randint(1, S.n_symbols, (B, T), generator=g)
    ref = torch.randn(B, 3000, generator=g) * 0.1
    kw = dict(steps=2, cfg_scale=5.0, noise=torch.randn(B, S.L_s, S.code_dim, generator=g),
              durations=torch.full((B, T), 2, dtype=torch.int32), seeds=[0, 1], check=False)
    bank = VoiceBank(eng, 2)
    rows = eng.voice_rows(B, bank, [bank.add(_voice(eng, 0)), bank.add(_voice(eng, 1))])

    def names(fn):
        del lib.calls[:]
        fn()
        return [c[0] for c in lib.calls]
    a = names(lambda: eng.synth(tok, ref, **kw))
    b = names(lambda: eng.synth(tok, None, voices=rows, **kw))
    i0, i1 = a.index("stzs_stft_frames"), a.index("stzs_code_quantize")
    assert b == a[:i0] + ["stzs_voice_prompt"] + a[i1 + 1:]
    mixed = eng.voice_rows(B, bank, [[0, 1], [1]], [[1, 3], None])
    del lib.calls[:]
    eng.synth(tok, None, voices=mixed, **kw)
    c = [x for x in lib.calls if x[0] == "stzs_voice_prompt"]
    assert len(c) == 1 and c[0][1]["gather"] == 0 and c[0][1]["Kmax"] == 2 and c[0][1]["B"] == B
    assert "ibank" in c[0][1] and "zmix" not in c[0][1]  # (optional pointers: recorded only when set)


def test_bank_save_load_and_fingerprint(host, tmp_path):
    from stzs.voice import Voice, VoiceBank
    eng, other, _ = host
    assert eng.voice_fingerprint() != other.voice_fingerprint()
    assert eng.voice_fingerprint() == eng.twin().voice_fingerprint()
    bank = VoiceBank(eng, 5)
    vs = [_voice(eng, s) for s in range(3)]
    for v in vs:
        bank.add(v)
    path = str(tmp_path / "voices.safetensors")
    bank.save(path)
    back = VoiceBank.load(path, eng)
    assert len(back) == 3 and back.capacity == 5 and back.meta == bank.meta
    for i, v in enumerate(vs):
        got = back.voice(i)
        assert got.z.numpy().tobytes() == v.z.numpy().tobytes() and got.idx.numpy().tobytes() == v.idx.numpy().tobytes()
        assert (got.clips, got.frontend, got.fingerprint) == (v.clips, v.frontend, eng.voice_fingerprint())
    with pytest.raises(ValueError):
        VoiceBank.load(path, other)
    with pytest.raises(ValueError):
        VoiceBank(other, 2).add(vs[0])
    with pytest.raises(ValueError):
        bank.replace(0, Voice(vs[0].z, vs[0].idx, other.voice_fingerprint()))
    with pytest.raises(ValueError):
        bank.replace(3, vs[0])  # not an added voice
    pz, pi = bank.z.data_ptr(), bank.idx.data_ptr()
    bank.replace(1, vs[2])
    assert torch.equal(bank.z[1], vs[2].z) and torch.equal(bank.idx[1], vs[2].idx)
    assert (pz, pi) == (bank.z.data_ptr(), bank.idx.data_ptr())
    small = VoiceBank(eng, 1)
    small.add(vs[0])
    with pytest.raises(ValueError):
        small.add(vs[1])
    from safetensors.torch import save_file
    save_file({"z": vs[0].z[None], "idx": vs[0].idx[None]}, path, metadata={"format": "something-else"})
    with pytest.raises(ValueError):
        VoiceBank.load(path, eng)


# ------------------------------------------------------------------ scheduler grouping
def test_phase1_groups_with_voices(host, tiny):
    from stzs.scheduler import BucketScheduler, Request, Stats
    eng, _, _ = host
    S = tiny
    va, vb = _voice(eng, 0), _voice(eng, 1)
    eps = torch.zeros(S.L_s, S.code_dim)
    tok = lambda n: torch.ones(n, dtype=torch.int32)
    wav = lambda n: torch.zeros(n)
    voiced = [Request(tok(n), None, eps, voice=v) for n, v in zip([5, 6, 7, 8, 5, 6], [va, vb, va, vb, vb, va])]
    sch = BucketScheduler(eng, max_batch=8, ragged_text=True)
    assert sch.phase1_groups(voiced) == [(False, [0, 1, 2, 3, 4, 5])]  # four token counts, two voices: one group
    assert BucketScheduler(eng, max_batch=4, ragged_text=True).phase1_groups(voiced) == [(False, [0, 1, 2, 3]),
                                                                                         (False, [4, 5])]
    assert BucketScheduler(eng, max_batch=8).phase1_groups(voiced) == [(False, [0, 4]), (False, [1, 5]), (False, [2]),
                                                                       (False, [3])]
    plain = [Request(tok(5), wav(3000), eps), Request(tok(5), wav(4000), eps), Request(tok(6), wav(3000), eps),
             Request(tok(5), wav(3000), eps, durations=torch.ones(5, dtype=torch.int32))]
    blend = Request(tok(5), None, eps, voice=[(va, 1.0), (vb, 3.0)])
    for flags in (dict(), dict(ragged_text=True), dict(ragged_ref=True), dict(ragged_text=True, ragged_ref=True)):
        sch = BucketScheduler(eng, max_batch=8, **flags)
        alone = sch.phase1_groups(plain)
        mixed = sch.phase1_groups([voiced[0], plain[0], plain[1], voiced[4], blend, plain[2], plain[3]])
        is_voice = [True, False, False, True, True, False, False]
        for _, ch in mixed:
            assert len({is_voice[i] for i in ch}) == 1, (flags, mixed)  # never voices and waveforms in one group
        assert [ch for _, ch in mixed if is_voice[ch[0]]] == [[0, 3, 4]], (flags, mixed)
        # the waveform requests among them group as they do alone (and that is today's grouping: the key is unchanged)
        order = [1, 2, 5, 6]
        assert [(f, [order.index(i) for i in ch]) for f, ch in mixed if not is_voice[ch[0]]] == alone
    assert BucketScheduler(eng).phase1_groups(plain) == [(False, [0]), (False, [1]), (False, [2]), (True, [3])]
    assert BucketScheduler(eng, ragged_text=True, ragged_ref=True).phase1_groups(plain) == [(False, [0, 1, 2]), (True, [3])]
    for bad in (Request(tok(5), wav(3000), eps, voice=va), Request(tok(5), None, eps),
                Request(tok(5), None, eps, voice=[]), Request(tok(5), None, eps, voice=[(va, 1.0), ("x", 1.0)]),
                Request(tok(5), None, eps, voice=va, ref_sr=16000)):
        with pytest.raises(ValueError):
            BucketScheduler(eng).phase1_groups([bad])
    assert "voice_batches" in Stats.OPTIONAL and Stats()["voice_batches"] == 0


# ------------------------------------------------------------------ the reference's own properties
def test_mix_ref_properties():
    """what makes the GPU cases exact: one source at weight 1 and a row blended with itself at (0.5, 0.5) or
    (0.25, 0.25, 0.5) are the row, bit for bit (powers of two: every product and every partial sum is exact, short
    of underflow)"""
    rng = np.random.default_rng(0)
    z = rng.standard_normal((3, 8, 32)).astype(np.float32)
    z[1, 0, :4] = [0.0, -0.0, np.float32(1e-30), np.float32(-3e30)]  # signed zeros, a tiny and a huge value
    same = lambda a, b: a.tobytes() == b.tobytes()
    src = np.array([[1, 1, 1]])
    assert same(mix_ref(z, src[:, :1], np.ones((1, 1), np.float32), [1])[0], z[1])
    half = mix_ref(z, src[:, :2], np.array([[0.5, 0.5]], np.float32), [2])[0]
    tri = mix_ref(z, src, np.array([[0.25, 0.25, 0.5]], np.float32), [3])[0]
    assert same(half, z[1]) and same(tri, z[1])
    # clamps, and entries past cnt never read
    w = np.array([[0.5, np.nan, np.nan]], np.float32)
    assert same(mix_ref(z, np.array([[-3, 99, 99]]), w, [0])[0], np.float32(0.5) * z[0])
    assert same(mix_ref(z, np.array([[10, 0, 0]]), np.array([[1, 1, 1]], np.float32), [5])[0],
                (np.float32(1) * z[2] + np.float32(1) * z[0]) + np.float32(1) * z[0])
    out = mix_ref(z, np.array([[0, 1, 2], [2, 1, 0]]), np.array([[0.3, 0.7, 0], [1, 2, 3]], np.float32), [2, 3])
    assert out.dtype == np.float32 and out.shape == (2, 8, 32)
    a = np.float32(0.3) * z[0]
    assert same(out[0], a + np.float32(0.7) * z[1])


def test_voice_prompt_operator_is_registered_with_its_fake(tiny):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from stzs import ops
    from stzs.engine import StyleTTSZS
    S = tiny
    assert "voice_prompt" in ops.OPS and hasattr(torch.ops.stzs, "voice_prompt")
    eng = object.__new__(StyleTTSZS)  # metadata-only stand-in: the fake only reads .spec
    eng.spec = S
    h = ops.register(eng)
    G = S.code_dim // S.vq_group
    with FakeTensorMode():
        zb, ib = torch.empty(5, S.L_s, S.code_dim), torch.empty(5, S.L_s, G, dtype=torch.int32)
        src, w, cnt = torch.empty(3, 2, dtype=torch.int32), torch.empty(3, 2), torch.empty(3, dtype=torch.int32)
        for ibank in (None, ib):
            i, q = torch.ops.stzs.voice_prompt(h, zb, ibank, src, w, cnt)
            assert i.shape == (3, S.L_s, G) and i.dtype == torch.int32
            assert q.shape == (3, S.L_s, S.code_dim) and q.dtype == torch.float32
    with pytest.raises(NotImplementedError):  # HIP-only: a CPU tensor raises, no fallback
        torch.ops.stzs.voice_prompt(h, torch.zeros(1, S.L_s, S.code_dim), None, torch.zeros(1, 1, dtype=torch.int32),
                                    torch.ones(1, 1), torch.ones(1, dtype=torch.int32))
