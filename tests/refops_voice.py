"""numpy float32 restatement of stzs_voice_prompt's mix (include/stzs.h) and the oracle's product VQ
behind it.  Every product and every sum below is one float32 operation, in the order the header states, so the bits
are the kernel's."""
import numpy as np
import torch


def mix_ref(zbank, src, w, cnt):
    """zbank float32 [V, L, C], src int [B, Kmax], w float32 [B, Kmax], cnt int [B] -> float32 [B, L, C]:
    n = clamp(cnt[b], 1, Kmax), s_k = clamp(src[b, k], 0, V - 1);
    acc = w[b, 0] * z[s_0]; acc = acc + (w[b, k] * z[s_k]) for k = 1 .. n - 1.  Entries k >= n are never read."""
    z = np.asarray(zbank, dtype=np.float32)
    src, cnt = np.asarray(src), np.asarray(cnt)
    w = np.asarray(w, dtype=np.float32)
    V = z.shape[0]
    B, Kmax = src.shape
    out = np.empty((B,) + z.shape[1:], dtype=np.float32)
    for b in range(B):
        n = min(max(int(cnt[b]), 1), Kmax)
        s = [min(max(int(src[b, k]), 0), V - 1) for k in range(n)]
        acc = np.float32(w[b, 0]) * z[s[0]]
        for k in range(1, n):
            acc = acc + np.float32(w[b, k]) * z[s[k]]
        assert acc.dtype == np.float32
        out[b] = acc
    return out


def vq_ref(codebook, z):
    """the oracle's product VQ (oracle/stzs_ref.py quantize_codes / lookup_codes, as tests/test_gpu_frontend.py uses
    them) of z [B, L, C] under codebook [G, K, dg] -> (idx int32 [B, L, G], q float32 [B, L, C]), torch tensors"""
    from oracle import stzs_ref as R
    P = {"pe.vq": torch.as_tensor(np.asarray(codebook, dtype=np.float32))}
    zt = torch.as_tensor(np.asarray(z, dtype=np.float32))
    idx, q, _ = R.quantize_codes(P, None, zt)
    assert torch.equal(q, R.lookup_codes(P, None, idx))
    return idx, q
