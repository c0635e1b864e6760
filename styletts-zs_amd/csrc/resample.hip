// Sample-rate conversion: stzs_resample, a rational polyphase FIR on caller-supplied tables.
//   y[b, j] = sum_{k < K} h[p, k] * X_b[q M + o[p] + k],  j = q L + p
// One 256-thread workgroup per (row, tile of RS_TILE consecutive outputs).  The tile's input span -- the
// ceil(RS_TILE M / L) + K samples from its first output's first tap on -- is staged once into LDS with the zero rule
// applied there (absolute index below 0, at or past the row's sample count, or outside the caller's window: +0.0f,
// the memory never loaded), the table beside it where both fit 64 KB.  Every output is then ONE fmaf chain over its K
// taps, k ascending, from +0.0f, whatever tile it falls into and wherever that tile starts: no interior fast path, so
// any split of the output range and any window of the input give the bits of the whole.
//
// LDS banking (ds_read_b32: bank = dword address % 32 within a 32-lane half): consecutive lanes hold consecutive
// outputs, i.e. consecutive phases p.  At the table's own pitch K4 (a multiple of 4 floats) the phases p and p + 8
// (K4 = 72: + 4) share a bank for every k; the LDS copy's pitch is K4 + 1, odd, so 32 consecutive phases sit on 32
// banks.  The span reads advance by about M / L samples per lane: conflict-free when upsampling (neighbours share or
// follow each other), up to M / L-way when downsampling -- left so, this is no throughput kernel.
//
// Built without packed-fp32 ops (build.py NO_PK): four independent fp32 FMA chains per thread are where hipcc pairs
// lanes' work into v_pk_fma_f32 with swapped operand halves (tests/test_isa_audit.py).
#include "common.hpp"

#define RS_TILE 1024
#define RS_THREADS 256
#define RS_LDS_MAX (64 * 1024)

template <bool PCM>
STZS_DEV void rs_store(void* y, long i, float v) {
    if (PCM) {
        // 32768 v is exact (a power of two); rintf: ties to even; the clamp holds NaN at -32768
        const float r = fminf(fmaxf(rintf(v * 32768.f), -32768.f), 32767.f);
        reinterpret_cast<int16_t*>(y)[i] = (int16_t)(int)r;
    } else {
        reinterpret_cast<float*>(y)[i] = v;
    }
}

// span: floats of the staged input span (ceil(RS_TILE M / L) + K); pitch: floats per phase of the LDS table copy
template <bool TAB_LDS, bool PCM>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const stzs_resample_args a, int span, int pitch) {
    extern __shared__ float rs_lds[];
    float* xs = rs_lds;         // [span]
    float* hs = rs_lds + span;  // [L][pitch] (TAB_LDS)
    const int b = blockIdx.y, tid = threadIdx.x;
    const int L = a.L, M = a.M, K = a.K, K4 = (K + 3) & ~3;

    // the row's sample count, clamped BEFORE it bounds anything (the product in 64 bits), and its output count
    long n_b = a.n_total;
    if (a.lens) {
        const long v = (long)a.lens[b] * (long)a.lens_mul;
        n_b = v < 0 ? 0 : (v > a.n_total ? a.n_total : v);
    }
    const long olen = (n_b * L + M - 1) / M;
    if (blockIdx.x == 0 && tid == 0 && a.out_lens) a.out_lens[b] = olen > 0x7fffffffL ? 0x7fffffff : (int)olen;

    const long jt = a.j0 + (long)blockIdx.x * RS_TILE;  // the tile's first output
    const int nj = (int)(a.j1 - jt < RS_TILE ? a.j1 - jt : RS_TILE);
    if (nj <= 0) return;  // (an empty launch keeps one workgroup per row for out_lens)
    const long yrow = (long)b * a.bsy + (jt - a.j0);
    if (jt >= olen) {  // the whole tile lies past the row's end: exact zeros, nothing read
        for (int d = tid; d < nj; d += RS_THREADS) rs_store<PCM>(a.y, yrow + d, 0.f);
        return;
    }
    const long qt = jt / L;
    const int pt = (int)(jt - qt * L);
    const long s0 = qt * M + a.o[pt];  // absolute index of the span's first sample

    const float* X = a.x + (long)b * a.bsx;
    for (int i = tid; i < span; i += RS_THREADS) {
        const long ab = s0 + i, w = ab - a.x0;
        float v = 0.f;
        if (ab >= 0 && ab < n_b && w >= 0 && w < a.n_x) v = X[w];
        xs[i] = v;
    }
    if (TAB_LDS) {
        const int kv = K4 >> 2, nv = L * kv;
        for (int v = tid; v < nv; v += RS_THREADS) {
            const int p = v / kv, k = (v - p * kv) * 4;
            const float4 q = reinterpret_cast<const float4*>(a.h)[v];
            float* d = hs + p * pitch + k;
            d[0] = q.x, d[1] = q.y, d[2] = q.z, d[3] = q.w;
        }
    }
    __syncthreads();

#pragma unroll 1
    for (int d = tid; d < nj; d += RS_THREADS) {
        const int pd = pt + d, dq = pd / L, p = pd - dq * L;  // output jt + d = (qt + dq) L + p
        long r = (long)dq * M + a.o[p] - a.o[pt];             // its first tap in the span
        r = r < 0 ? 0 : (r > span - K ? span - K : r);        // (a table that is not monotone: clamped, never out of bounds)
        const float* xp = xs + r;
        float acc = 0.f;
        if (TAB_LDS) {
            const float* hp = hs + p * pitch;
            for (int k = 0; k < K; ++k) acc = fmaf(hp[k], xp[k], acc);
        } else {
            const float* hp = a.h + (long)p * K4;
            for (int k = 0; k < K; ++k) acc = fmaf(hp[k], xp[k], acc);
        }
        rs_store<PCM>(a.y, yrow + d, jt + d < olen ? acc : 0.f);
    }
}

extern "C" int stzs_resample(const stzs_resample_args* a, void* stream) {
    if (!a || !a->x || !a->h || !a->o || !a->y) return STZS_EINVAL;
    if (a->out_dtype != STZS_F32 && a->out_dtype != STZS_I16) return STZS_EINVAL;
    if (!stzs_aligned(a->h, 16) || !stzs_aligned(a->x, 4) || !stzs_aligned(a->o, 4) || !stzs_aligned(a->lens, 4) ||
        !stzs_aligned(a->out_lens, 4) || !stzs_aligned(a->y, a->out_dtype == STZS_I16 ? 2 : 4))
        return STZS_EINVAL;
    const int64_t lim = (int64_t)1 << 50;  // (sample counts far below the 64-bit products' range)
    if (a->L < 1 || a->L > 1024 || a->M < 1 || a->M > 1024 || a->K < 1 || a->K > 512 || a->M > 8 * a->L)
        return STZS_ESHAPE;
    if (a->B < 1 || a->B > 65535 || a->j0 < 0 || a->j1 < a->j0 || a->j1 > lim || a->n_x < 0 || a->n_total < 0 ||
        a->n_total > lim || a->x0 < -lim || a->x0 > lim || a->bsx < a->n_x || a->bsy < a->j1 - a->j0)
        return STZS_ESHAPE;
    const int64_t tiles = (a->j1 - a->j0 + RS_TILE - 1) / RS_TILE;
    if (tiles > 0x7fffffffLL) return STZS_ESHAPE;
    const int K4 = (a->K + 3) & ~3, pitch = K4 + 1;
    const int span = (RS_TILE * a->M + a->L - 1) / a->L + a->K;  // <= 8192 + 512 floats
    const size_t lx = (size_t)span * 4, lt = (size_t)a->L * pitch * 4;
    const bool tab = lx + lt <= RS_LDS_MAX;
    const bool pcm = a->out_dtype == STZS_I16;
    const dim3 grid((unsigned)(tiles > 0 ? tiles : 1), a->B), block(RS_THREADS);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (tab)
        return pcm ? stzs_launch(resample_kernel<true, true>, grid, block, lx + lt, s, *a, span, pitch)
                   : stzs_launch(resample_kernel<true, false>, grid, block, lx + lt, s, *a, span, pitch);
    return pcm ? stzs_launch(resample_kernel<false, true>, grid, block, lx, s, *a, span, pitch)
               : stzs_launch(resample_kernel<false, false>, grid, block, lx, s, *a, span, pitch);
}
