// Enrolled voices: stzs_voice_prompt, one launch from a device-resident voice bank and per-row sources
// to the prompt rows sample_style consumes.  A voice is the pre-quantiser prompt features z [L, code] of its
// reference clip(s) and their product-VQ indices [L, G]; row (b, l) of the batch is
//   mix form    acc = w[b,0] z[s_0][l];  acc = acc + (w[b,k] z[s_k][l]) for k = 1 .. n-1, every product and every sum
//               rounded to fp32 on its own, then the product VQ of acc;
//   gather form idx = ibank[s_0][l], y = the codebook rows: rows the host knows to be one voice at weight 1.
// src, w and cnt are device arrays read by the kernel (clamped before they bound anything), so a captured graph
// replays for other speakers after they are rewritten in place.
//
// The scan is stzs_code_quantize's (csrc/frontend.hip vq_kernel), restated: one workgroup per (64 rows, group), the
// group's codebook staged in LDS, the K entries split over 4 waves, the distance summed serially over j with
// separately rounded sub / mul / add, strict < inside a wave's range and across the ranges in range order -- the first
// global minimum.  This file is built with -ffp-contract=off (build.py FILE_FLAGS): under the library's
// -ffp-contract=fast the backend fuses w z + acc and t t + d into one rounding, which is not the definition.
//
// Built without packed-fp32 ops (build.py NO_PK): the mix is DG independent mul / add chains per lane, the shape hipcc
// pairs into v_pk_mul_f32 / v_pk_add_f32 with swapped operand halves (tests/test_isa_audit.py).
#include "common.hpp"

namespace {

constexpr int VP_WAVES = 4;
constexpr int VP_KMAX = 8;

STZS_DEV int vp_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int DG>
__global__ __launch_bounds__(64 * VP_WAVES) void voice_mix_kernel(const stzs_voice_args a) {
    extern __shared__ __attribute__((aligned(16))) float cbs[];  // [K][DG], then [VP_WAVES][64] (d, k) pairs
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long R = (long)a.B * a.L;
    const long r = (long)blockIdx.x * 64 + lane;
    const int g = blockIdx.y;
    const float* cb = a.codebook + (long)g * a.K * DG;
    const bool row_ok = r < R;
    for (int e = threadIdx.x; e < a.K * DG; e += 64 * VP_WAVES) cbs[e] = cb[e];
    float x[DG];
#pragma unroll
    for (int j = 0; j < DG; ++j) x[j] = 0.f;
    if (row_ok) {
        const int b = (int)(r / a.L), l = (int)(r - (long)b * a.L);
        const int n = vp_clamp(a.cnt[b], 1, a.Kmax);
        const int32_t* S = a.src + (long)b * a.Kmax;
        const float* Wt = a.w + (long)b * a.Kmax;
        for (int k = 0; k < n; ++k) {  // (entries k >= n of src and w are never read)
            const int s = vp_clamp(S[k], 0, a.V - 1);
            const float wk = Wt[k];
            const float* Z = a.zbank + ((long)s * a.L + l) * a.ldz + g * DG;
#pragma unroll
            for (int j = 0; j < DG; ++j) {
                const float p = wk * Z[j];
                x[j] = k == 0 ? p : x[j] + p;
            }
        }
        if (w == 0 && a.zmix) {
            float* M = a.zmix + r * a.ldm + g * DG;
#pragma unroll
            for (int j = 0; j < DG; ++j) M[j] = x[j];
        }
    }
    __syncthreads();
    const int per = (a.K + VP_WAVES - 1) / VP_WAVES;
    const int k0 = w * per, k1 = min(a.K, k0 + per);
    float bd = __builtin_inff();
    int best = k0 < k1 ? k0 : 0;
    for (int k = k0; k < k1; ++k) {
        const float* c = cbs + k * DG;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < DG; ++j) {
            const float t = x[j] - c[j];
            const float q = t * t;
            d = d + q;
        }
        if (d < bd) {
            bd = d;
            best = k;
        }
    }
    float* pd = cbs + a.K * DG;
    int* pk = reinterpret_cast<int*>(pd + VP_WAVES * 64);
    pd[w * 64 + lane] = bd;
    pk[w * 64 + lane] = best;
    __syncthreads();
    if (w != 0 || !row_ok) return;
    float gd = pd[lane];
    int gb = pk[lane];
#pragma unroll
    for (int q = 1; q < VP_WAVES; ++q)
        if (pd[q * 64 + lane] < gd) {
            gd = pd[q * 64 + lane];
            gb = pk[q * 64 + lane];
        }
    a.idx[r * a.ldi + g] = gb;
    const float* c = cbs + gb * DG;
    float* Y = a.y + r * a.ldy + g * DG;
#pragma unroll
    for (int j = 0; j < DG; ++j) Y[j] = c[j];
}

// one thread per (row, group): no LDS, no barrier, no scan.  The stored index is clamped into [0, K) before it
// addresses the codebook (a bank holds what the mix form wrote, so the clamp changes nothing there).
template <int DG>
__global__ __launch_bounds__(64) void voice_gather_kernel(const stzs_voice_args a) {
    const long R = (long)a.B * a.L;
    const long r = (long)blockIdx.x * 64 + threadIdx.x;
    const int g = blockIdx.y;
    if (r >= R) return;
    const int b = (int)(r / a.L), l = (int)(r - (long)b * a.L);
    const int s = vp_clamp(a.src[(long)b * a.Kmax], 0, a.V - 1);
    const long br = (long)s * a.L + l;
    const int k = vp_clamp(a.ibank[br * a.ldib + g], 0, a.K - 1);
    a.idx[r * a.ldi + g] = k;
    const float* c = a.codebook + ((long)g * a.K + k) * DG;
    float* Y = a.y + r * a.ldy + g * DG;
#pragma unroll
    for (int j = 0; j < DG; ++j) Y[j] = c[j];
    if (a.zmix) {
        const float* Z = a.zbank + br * a.ldz + g * DG;
        float* M = a.zmix + r * a.ldm + g * DG;
#pragma unroll
        for (int j = 0; j < DG; ++j) M[j] = Z[j];
    }
}

}  // namespace

extern "C" int stzs_voice_prompt(const stzs_voice_args* a, void* stream) {
    if (!a || !a->zbank || !a->codebook || !a->src || !a->w || !a->cnt || !a->idx || !a->y) return STZS_EINVAL;
    if (a->gather && !a->ibank) return STZS_EINVAL;
    if (!stzs_aligned(a->zbank, 4) || !stzs_aligned(a->ibank, 4) || !stzs_aligned(a->codebook, 4) ||
        !stzs_aligned(a->src, 4) || !stzs_aligned(a->w, 4) || !stzs_aligned(a->cnt, 4) || !stzs_aligned(a->idx, 4) ||
        !stzs_aligned(a->y, 4) || !stzs_aligned(a->zmix, 4))
        return STZS_EINVAL;
    if (a->V <= 0 || a->L <= 0 || a->B <= 0 || a->G <= 0 || a->K <= 0 || a->Kmax <= 0 || a->Kmax > VP_KMAX)
        return STZS_ESHAPE;
    if (a->G > 65535 || (int64_t)a->B * a->L > 0x7fffffffLL - 64 || (int64_t)a->V * a->L > 0x7fffffffLL)
        return STZS_ESHAPE;
    if (a->dg != 4 && a->dg != 8 && a->dg != 16) return STZS_ESHAPE;
    const int64_t C = (int64_t)a->G * a->dg;
    if (a->ldz < C || a->ldi < a->G || a->ldy < C || (a->zmix && a->ldm < C) || (a->gather && a->ldib < a->G))
        return STZS_ESHAPE;
    const size_t lds = (size_t)a->K * a->dg * 4 + VP_WAVES * 64 * 8;
    if (lds > 64 * 1024) return STZS_ESHAPE;  // codebook of one group staged in LDS (the mix form; one limit for both)
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 g((unsigned)(((int64_t)a->B * a->L + 63) / 64), a->G);
    if (a->gather) {
        switch (a->dg) {
            case 4: return stzs_launch(voice_gather_kernel<4>, g, dim3(64), 0, s, *a);
            case 8: return stzs_launch(voice_gather_kernel<8>, g, dim3(64), 0, s, *a);
            default: return stzs_launch(voice_gather_kernel<16>, g, dim3(64), 0, s, *a);
        }
    }
    switch (a->dg) {
        case 4: return stzs_launch(voice_mix_kernel<4>, g, dim3(64 * VP_WAVES), lds, s, *a);
        case 8: return stzs_launch(voice_mix_kernel<8>, g, dim3(64 * VP_WAVES), lds, s, *a);
        default: return stzs_launch(voice_mix_kernel<16>, g, dim3(64 * VP_WAVES), lds, s, *a);
    }
}
