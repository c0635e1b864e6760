// Precise reference-prompt log-mel in ONE launch (StyleTTSZS(precise_frontend=True)): windowed frame -> fp32 real FFT
// in LDS -> power -> sparse mel filterbank -> log, one workgroup per (frame, utterance).  It restates the three launches
// of csrc/frontend.hip (stzs_stft_frames -> bf16 DFT GEMM -> stzs_log_mel) with every value in fp32, so the log-mel
// agrees with the fp32 oracle (oracle/stzs_ref.py log_mel: torch.stft) to fp32 rounding instead of the 1.2e-3 of the
// bf16 DFT.
//
// The n_fft-point real transform is an M = n_fft / 2 point complex one of the packed sequence z[n] = x[2n] + i x[2n+1]
// (Stockham autosort, radix-4 stages and one radix-2 stage when log2(M) is odd, ping-pong between two LDS buffers),
// followed by the split step X[k] = E[k] + w^k O[k], E = (Z[k] + conj Z[M-k]) / 2, O = (Z[k] - conj Z[M-k]) / 2i.
// Twiddles come only from the host table w^q = (cos, -sin)(2 pi q / n_fft), q < n_fft, computed in float64 and
// rounded once (stzs/weights.py stft_twiddles): no device trigonometry, every product and sum written out with fmaf,
// so the bits do not depend on contraction choices.
//
// LDS layout: re / im planes of M floats per buffer, element i at i ^ swz(i) -- the XOR of i's bits 5-6 into bits 0-4
// below.  A radix-4 stage reads in[j + r M/4] (consecutive lanes, consecutive words) and writes
// out[4 Ns (j / Ns) + j % Ns + r Ns]: at Ns = 1, 4, 16 the 32 lanes of a half wave would land on 8, 8 and 16 distinct
// banks (4-, 4- and 2-way conflicts of ds_write_b32, bank = word % 32); the swizzle spreads every stage's reads and
// writes over 32 distinct banks (conflict-free by the bank rule for M >= 64; the split step's reversed read Z[M - k]
// straddles two 32-word blocks: 2-way, once per frame).  The swizzle permutes words inside aligned 32-word blocks, so
// no padding is needed.
#include "common.hpp"

namespace {

constexpr int FT = 256;

STZS_DEV int fswz(int i) {
    const int b = (i >> 5) & 3;
    return i ^ (b | (b << 2) | ((b >> 1) << 4));
}

// (xr + i xi) * (wr + i wi), each part one product rounded and one fma
STZS_DEV void cmul(float xr, float xi, float wr, float wi, float& yr, float& yi) {
    yr = fmaf(xr, wr, -(xi * wi));
    yi = fmaf(xr, wi, xi * wr);
}

template <typename TO>
__global__ __launch_bounds__(FT) void stft_logmel_kernel(const stzs_stftmel_args a) {
#pragma clang fp contract(off)
    extern __shared__ float sm[];
    const int tid = threadIdx.x;
    const int t = blockIdx.x, b = blockIdx.y;
    const int n_fft = a.n_fft, M = n_fft >> 1;
    float* sr = sm;  // source buffer (re | im), then the destination one, then the power spectrum [M + 1]
    float* si = sm + M;
    float* dr = sm + 2 * M;
    float* di = sm + 3 * M;
    float* pw = sm + 4 * M;
    const float2* tw = reinterpret_cast<const float2*>(a.twiddle);

    // ragged batch: this utterance's own sample count, clamped into the range the reflection is defined on; a frame
    // past its last one is a row of zeros (the padding the prompt convs see) and its workgroup leaves here -- t and b
    // are the workgroup's, so the whole workgroup leaves, before any barrier
    int N = a.N;
    if (a.n_lens) {
        N = min(max(a.n_lens[b], M + 1), a.N);
        const int Fb = N / a.hop + 1;
        if (t == 0 && tid == 0 && a.f_lens_out) a.f_lens_out[b] = Fb;
        if (t >= Fb) {
            TO* Z = reinterpret_cast<TO*>(a.y) + (long)b * a.bsy + (long)t * a.ldy;
            for (int m = tid; m < a.n_mels; m += FT) DT<TO>::st(Z + m, 0.f);
            return;
        }
    }

    // the frame as stzs_stft_frames defines it: torch.stft(center=True, pad_mode="reflect"), the window centred in n_fft
    // (the final clamp only keeps a frame count beyond N / hop + 1 inside the row)
    const float* X = a.wav + (long)b * a.ldw;
    const int off = (n_fft - a.win) / 2;
    for (int m = tid; m < n_fft; m += FT) {
        float v = 0.f;
        const int mw = m - off;
        if (mw >= 0 && mw < a.win) {
            long j = (long)t * a.hop + m - n_fft / 2;
            if (j < 0) j = -j;
            if (j >= N) j = 2L * (N - 1) - j;
            j = j < 0 ? 0 : (j >= N ? N - 1 : j);
            v = a.window[mw] * X[j];
        }
        ((m & 1) ? si : sr)[fswz(m >> 1)] = v;
    }
    __syncthreads();

    int Ns = 1;
    for (; Ns * 4 <= M; Ns *= 4) {
        const int Q = M >> 2;
        const int tstep = n_fft / (Ns * 4);  // w_{4 Ns}^k = tw[k * tstep]
        for (int j = tid; j < Q; j += FT) {
            const int k = j & (Ns - 1);
            float vr[4], vi[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = fswz(j + r * Q);
                vr[r] = sr[p];
                vi[r] = si[p];
            }
            if (Ns > 1) {
#pragma unroll
                for (int r = 1; r < 4; ++r) {
                    const float2 w = tw[r * k * tstep];  // < 3 n_fft / 4
                    float yr, yi;
                    cmul(vr[r], vi[r], w.x, w.y, yr, yi);
                    vr[r] = yr;
                    vi[r] = yi;
                }
            }
            const float a0r = vr[0] + vr[2], a0i = vi[0] + vi[2];
            const float a1r = vr[0] - vr[2], a1i = vi[0] - vi[2];
            const float a2r = vr[1] + vr[3], a2i = vi[1] + vi[3];
            const float a3r = vi[1] - vi[3], a3i = -(vr[1] - vr[3]);  // -i (v1 - v3)
            const int j0 = ((j - k) << 2) + k;
            const int p0 = fswz(j0), p1 = fswz(j0 + Ns), p2 = fswz(j0 + 2 * Ns), p3 = fswz(j0 + 3 * Ns);
            dr[p0] = a0r + a2r;
            di[p0] = a0i + a2i;
            dr[p1] = a1r + a3r;
            di[p1] = a1i + a3i;
            dr[p2] = a0r - a2r;
            di[p2] = a0i - a2i;
            dr[p3] = a1r - a3r;
            di[p3] = a1i - a3i;
        }
        __syncthreads();
        float* x = sr; sr = dr; dr = x;
        x = si; si = di; di = x;
    }
    if (Ns < M) {  // log2(M) odd: one radix-2 stage, Ns = M / 2
        const int Q = M >> 1;
        for (int j = tid; j < Q; j += FT) {
            const int p = fswz(j), q = fswz(j + Q);
            const float2 w = tw[2 * j];  // w_M^j
            float yr, yi;
            cmul(sr[q], si[q], w.x, w.y, yr, yi);
            const float ur = sr[p], ui = si[p];
            dr[p] = ur + yr;  // (j < Ns: output index j, and j + Ns = j + Q)
            di[p] = ui + yi;
            dr[q] = ur - yr;
            di[q] = ui - yi;
        }
        __syncthreads();
        float* x = sr; sr = dr; dr = x;
        x = si; si = di; di = x;
    }

    // split step and power: bins 0 .. M
    for (int k = tid; k <= M; k += FT) {
        const int p = fswz(k & (M - 1)), q = fswz((M - k) & (M - 1));
        const float zr = sr[p], zi = si[p], cr = sr[q], ci = -si[q];  // Z[k], conj Z[M - k]
        const float er = 0.5f * (zr + cr), ei = 0.5f * (zi + ci);
        const float hr = 0.5f * (zr - cr), hi = 0.5f * (zi - ci);  // i O[k]
        const float2 w = tw[k];                                    // k <= n_fft / 2 < n_fft
        float yr, yi;
        cmul(hi, -hr, w.x, w.y, yr, yi);  // w^k O[k], O = -i (i O)
        const float re = er + yr, im = ei + yi;
        pw[k] = fmaf(re, re, im * im);
    }
    __syncthreads();

    // mel filterbank and log: stzs_log_mel's sums ([k0, k1) ranges, the same fmaf chain)
    const int nbin = M + 1;
    TO* Y = reinterpret_cast<TO*>(a.y) + (long)b * a.bsy + (long)t * a.ldy;
    for (int m = tid; m < a.n_mels; m += FT) {
        const int k0 = max(a.ranges[2 * m], 0), k1 = min(a.ranges[2 * m + 1], nbin);
        const float* w = a.fb + (long)m * nbin;
        float acc = 0.f;
        for (int k = k0; k < k1; ++k) acc = fmaf(w[k], pw[k], acc);
        DT<TO>::st(Y + m, logf(fmaxf(acc, 1e-5f)));
    }
}

}  // namespace

extern "C" int stzs_stft_logmel(const stzs_stftmel_args* a, void* stream) {
    if (!a || !a->wav || !a->window || !a->twiddle || !a->fb || !a->ranges || !a->y) return STZS_EINVAL;
    if (a->f_lens_out && !a->n_lens) return STZS_EINVAL;  // the frame counts are those of the ragged launch only
    if (a->B <= 0 || a->B > 65535 || a->N <= 0 || a->F <= 0 || a->n_fft <= 0 || a->win <= 0 || a->hop <= 0 ||
        a->n_mels <= 0)
        return STZS_ESHAPE;
    if (a->n_fft < 64 || a->n_fft > 4096 || (a->n_fft & (a->n_fft - 1))) return STZS_ESHAPE;
    if (a->win > a->n_fft || a->n_fft / 2 >= a->N) return STZS_ESHAPE;  // reflect padding needs N > n_fft / 2 (as torch)
    if ((long)(a->F - 1) * a->hop > (long)a->N + a->n_fft) return STZS_ESHAPE;
    if (a->ldy < a->n_mels || a->ldw < a->N) return STZS_ESHAPE;
    if (a->out_dtype != STZS_BF16 && a->out_dtype != STZS_F32) return STZS_EDTYPE;
    const int M = a->n_fft / 2;
    const size_t lds = ((size_t)4 * M + M + 1) * sizeof(float);  // <= 40 KB + 4 B at n_fft 4096
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (a->out_dtype == STZS_F32)
        return stzs_launch(stft_logmel_kernel<float>, dim3(a->F, a->B), dim3(FT), lds, s, *a);
    else
        return stzs_launch(stft_logmel_kernel<bf16_t>, dim3(a->F, a->B), dim3(FT), lds, s, *a);
}
