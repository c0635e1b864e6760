// Sampler glue and small utilities + library entry points.
//   stzs_dn_cond      c = silu(pooled prompt + sigma embedding)        (adaLN-single input)
//   stzs_adaln_expand per-layer modulation = shared + table[l] (+1 on scale chunks)
//   stzs_cfg_euler    fused classifier-free guidance combine + Euler step, fp32 state
//   stzs_cfg_euler_rows  the same with one guidance scale per row (per-request controls)
//   stzs_state_init   x0 = eps * sigma_0 for the (duplicated) CFG state
//   stzs_mean_rows    pooled style / prompt vectors
//   stzs_copy2d       strided row copy with dtype conversion (buffer assembly, no torch ops)
//   stzs_embed        token embedding rows (text front end)
//   stzs_frame_rows   the ragged decoder's per-stage row counts from the alignment's frame counts
//   stzs_row_scale    x[b, :] *= mul[b] (the per-row pitch factor on F0)
#include "common.hpp"
#include "cfg.hpp"

namespace {

// c[s][r][j] = silu(pool[r][j] + temb[s][j]) for all sampler steps s at once
template <typename TO>
__global__ void dn_cond_kernel(const float* pool, const float* temb, TO* c, int R, int D, int steps) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long rd = (long)R * D;
    if (i >= rd * steps) return;
    const int s = (int)(i / rd);
    const long rj = i - s * rd;
    const int j = (int)(rj % D);
    const float x = pool[rj] + temb[(long)s * D + j];
    DT<TO>::st(c + i, x / (1.f + expf(-x)));
}

__global__ void adaln_expand_kernel(const float* mod, const float* table, float* out, int R, int D, int nchunk,
                                    int nlayers, unsigned mask) {
    const long W = (long)nchunk * D;
    const long n = (long)nlayers * R * W;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long l = i / (R * W);
    const long rem = i - l * R * W;
    const long j = rem % W;
    float v = mod[rem];
    if (table) v += table[l * W + j];
    if ((mask >> (j / D)) & 1u) v += 1.f;
    out[i] = v;
}

__global__ void cfg_euler_kernel(float* x, const float* D, int B, int N, int cfg, float s, float s0, float dsig) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * N) return;
    const float xn = stzs_cfg_euler_elem(x[i], D[i], cfg ? D[(long)B * N + i] : 0.f, cfg, s, s0, dsig);
    x[i] = xn;
    if (cfg) x[(long)B * N + i] = xn;
}

// one guidance scale per row, always on the duplicated state: a row whose scale is exactly 1 takes its D_c alone (the
// cfg = 0 expression on that row), every other row the CFG expression of stzs_cfg_euler_elem unchanged
__global__ void cfg_euler_rows_kernel(float* x, const float* D, int B, int N, const float* scales, float s0,
                                      float dsig) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * N) return;
    const float s = scales[i / N];
    const float xn = stzs_cfg_euler_elem(x[i], D[i], D[(long)B * N + i], s != 1.f, s, s0, dsig);
    x[i] = xn;
    x[(long)B * N + i] = xn;
}

// x[b, t] *= mul[b], t < T.  WIDE (the host found ld == 1 and base / bs multiples of 16 bytes): 4 elements per thread,
// a whole group as one 16-byte load and store, the row's last partial group element by element
template <bool WIDE>
__global__ __launch_bounds__(256) void row_scale_kernel(const stzs_row_scale_args a) {
    const int b = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    const float m = a.mul[b];
    float* X = a.x + (long)b * a.bs;
    if (WIDE) {
        const int t0 = v * 4;
        if (t0 >= a.T) return;
        if (t0 + 4 <= a.T) {
            float4 q = *reinterpret_cast<const float4*>(X + t0);
            q.x *= m, q.y *= m, q.z *= m, q.w *= m;
            *reinterpret_cast<float4*>(X + t0) = q;
        } else {
            for (int t = t0; t < a.T; ++t) X[t] *= m;
        }
    } else {
        if (v >= a.T) return;
        X[(long)v * a.ld] *= m;
    }
}

__global__ void state_init_kernel(float* x, const float* eps, int B, int N, int cfg, float sigma) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * N) return;
    const float v = eps[i] * sigma;
    x[i] = v;
    if (cfg) x[(long)B * N + i] = v;
}

// out[k][b] = clamp(lens[b], 1, T) * mul[k] + add[k]: the ragged decoder's row counts per stage (the clamp first, the
// arithmetic in 64 bits, the result saturated: a garbage length never wraps into range)
__global__ void frame_rows_kernel(const stzs_frame_rows_args a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.B * a.n) return;
    const int k = i / a.B, b = i - k * a.B;
    const long v = (long)rag_rows(a.lens, b, 1, a.T) * a.mul[k] + a.add[k];
    a.out[i] = v > 0x7fffffffL ? 0x7fffffff : (v < -0x7fffffffL - 1 ? -0x7fffffff - 1 : (int)v);
}

__global__ void mean_rows_kernel(const float* x, float* y, int B, int L, long ldx, long bsx, int c0, int C,
                                 long ldy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * C) return;
    const int b = (int)(i / C), c = (int)(i - (long)b * C);
    // 8 rows' loads in flight at a time, summed in row order (the serial loop waited on each load in turn)
    const float* X = x + b * bsx + c0 + c;
    float s = 0.f;
    int l = 0;
    for (; l + 8 <= L; l += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = X[(long)(l + j) * ldx];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; l < L; ++l) s += X[(long)l * ldx];
    y[b * ldy + c] = s / L;
}

template <typename TI, typename TO>
__global__ void copy_kernel(const stzs_copy_args a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)a.B * a.R * a.C;
    if (i >= n) return;
    const long c = i % a.C;
    const long rr = (i / a.C) % a.R;
    const long b = i / ((long)a.C * a.R);
    const float v = DT<TI>::ld(reinterpret_cast<const TI*>(a.x) + b * a.bsx + rr * a.ldx + c);
    const long ro = a.dst_row_off ? max(a.dst_row_off[b], 0) : 0;  // (the caller sizes y for its offsets)
    DT<TO>::st(reinterpret_cast<TO*>(a.y) + b * a.bsy + (ro + rr) * a.ldy + c, v);
}

template <typename TO>
__global__ void embed_kernel(const int32_t* tok, const float* emb, TO* y, int B, int T, int D, long ldy) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int id = tok[(long)b * T + t];
    const float* e = emb + (long)id * D;
    TO* o = y + ((long)b * T + t) * ldy;
    for (int c = threadIdx.x; c < D; c += 256) DT<TO>::st(o + c, e[c]);
}

// ragged batch: rows t >= lens[b] (clamped into [1, T]) are zeros, their tokens are not read
template <typename TO>
__global__ void embed_lens_kernel(const int32_t* tok, const float* emb, TO* y, const int32_t* lens, int B, int T,
                                  int D, long ldy) {
    const int t = blockIdx.x, b = blockIdx.y;
    const bool keep = t < min(max(lens[b], 1), T);  // uniform per workgroup
    const float* e = emb + (long)(keep ? tok[(long)b * T + t] : 0) * D;
    TO* o = y + ((long)b * T + t) * ldy;
    for (int c = threadIdx.x; c < D; c += 256) DT<TO>::st(o + c, keep ? e[c] : 0.f);
}

inline unsigned nblk(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int stzs_dn_cond(const float* pool, const float* temb, void* c, int R, int D, void* stream) {
    if (!pool || !temb || !c) return STZS_EINVAL;
    if (R <= 0 || D <= 0) return STZS_ESHAPE;
    return stzs_launch(dn_cond_kernel<bf16_t>, dim3(nblk((long)R * D)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       pool, temb, reinterpret_cast<bf16_t*>(c), R, D, 1);
}

extern "C" int stzs_dn_cond_steps(const float* pool, const float* temb, void* c, int R, int D, int steps,
                                  void* stream) {
    if (!pool || !temb || !c) return STZS_EINVAL;
    if (R <= 0 || D <= 0 || steps <= 0) return STZS_ESHAPE;
    return stzs_launch(dn_cond_kernel<bf16_t>, dim3(nblk((long)R * D * steps)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), pool, temb, reinterpret_cast<bf16_t*>(c), R, D, steps);
}

extern "C" int stzs_dn_cond_steps_f32(const float* pool, const float* temb, float* c, int R, int D, int steps,
                                      void* stream) {
    if (!pool || !temb || !c) return STZS_EINVAL;
    if (R <= 0 || D <= 0 || steps <= 0) return STZS_ESHAPE;
    return stzs_launch(dn_cond_kernel<float>, dim3(nblk((long)R * D * steps)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), pool, temb, c, R, D, steps);
}

extern "C" int stzs_adaln_expand(const float* mod, const float* table, float* out, int R, int D, int nchunk,
                                 int nlayers, unsigned scale_mask, void* stream) {
    if (!mod || !out) return STZS_EINVAL;
    if (R <= 0 || D <= 0 || nchunk <= 0 || nchunk > 32 || nlayers <= 0) return STZS_ESHAPE;
    return stzs_launch(adaln_expand_kernel, dim3(nblk((long)nlayers * R * nchunk * D)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), mod, table, out, R, D, nchunk, nlayers, scale_mask);
}

extern "C" int stzs_cfg_euler(float* x, const float* D, int B, int N, int cfg, float scale, float s0, float dsig,
                              void* stream) {
    if (!x || !D) return STZS_EINVAL;
    if (B <= 0 || N <= 0 || !(s0 > 0.f)) return STZS_ESHAPE;
    return stzs_launch(cfg_euler_kernel, dim3(nblk((long)B * N)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       x, D, B, N, cfg, scale, s0, dsig);
}

extern "C" int stzs_cfg_euler_rows(float* x, const float* D, int B, int N, const float* scales, float s0, float dsig,
                                   void* stream) {
    if (!x || !D || !scales) return STZS_EINVAL;
    if (B <= 0 || N <= 0 || !(s0 > 0.f)) return STZS_ESHAPE;
    return stzs_launch(cfg_euler_rows_kernel, dim3(nblk((long)B * N)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), x, D, B, N, scales, s0, dsig);
}

extern "C" int stzs_row_scale(const stzs_row_scale_args* a, void* stream) {
    if (!a || !a->x || !a->mul || !stzs_aligned(a->x, 4) || !stzs_aligned(a->mul, 4)) return STZS_EINVAL;
    if (a->B <= 0 || a->B > 65535 || a->T <= 0 || a->ld < 1 || a->bs < (int64_t)(a->T - 1) * a->ld + 1)
        return STZS_ESHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool wide = a->ld == 1 && reinterpret_cast<uintptr_t>(a->x) % 16 == 0 && a->bs % 4 == 0;
    if (wide) return stzs_launch(row_scale_kernel<true>, dim3(nblk((a->T + 3) / 4), a->B), dim3(256), 0, s, *a);
    return stzs_launch(row_scale_kernel<false>, dim3(nblk(a->T), a->B), dim3(256), 0, s, *a);
}

extern "C" int stzs_state_init(float* x, const float* eps, int B, int N, int cfg, float sigma, void* stream) {
    if (!x || !eps) return STZS_EINVAL;
    if (B <= 0 || N <= 0) return STZS_ESHAPE;
    return stzs_launch(state_init_kernel, dim3(nblk((long)B * N)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), x, eps, B, N, cfg, sigma);
}

extern "C" int stzs_mean_rows(const float* x, float* y, int B, int L, int64_t ldx, int64_t bsx, int c0, int C,
                              int64_t ldy, void* stream) {
    if (!x || !y) return STZS_EINVAL;
    if (B <= 0 || L <= 0 || C <= 0) return STZS_ESHAPE;
    return stzs_launch(mean_rows_kernel, dim3(nblk((long)B * C)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       x, y, B, L, (long)ldx, (long)bsx, c0, C, (long)ldy);
}

extern "C" int stzs_copy2d(const stzs_copy_args* a, void* stream) {
    if (!a || !a->x || !a->y) return STZS_EINVAL;
    if (a->B <= 0 || a->R <= 0 || a->C <= 0) return STZS_ESHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 g(nblk((long)a->B * a->R * a->C));
    if (a->in_dtype == STZS_F32 && a->out_dtype == STZS_F32)
        return stzs_launch((copy_kernel<float, float>), g, dim3(256), 0, s, *a);
    else if (a->in_dtype == STZS_F32 && a->out_dtype == STZS_BF16)
        return stzs_launch((copy_kernel<float, bf16_t>), g, dim3(256), 0, s, *a);
    else if (a->in_dtype == STZS_BF16 && a->out_dtype == STZS_BF16)
        return stzs_launch((copy_kernel<bf16_t, bf16_t>), g, dim3(256), 0, s, *a);
    else if (a->in_dtype == STZS_BF16 && a->out_dtype == STZS_F32)
        return stzs_launch((copy_kernel<bf16_t, float>), g, dim3(256), 0, s, *a);
    else
        return STZS_EDTYPE;
}

extern "C" int stzs_frame_rows(const stzs_frame_rows_args* a, void* stream) {
    if (!a || !a->lens || !a->out || !stzs_aligned(a->lens, 4) || !stzs_aligned(a->out, 4)) return STZS_EINVAL;
    if (a->B <= 0 || a->T <= 0 || a->n <= 0 || a->n > 8) return STZS_ESHAPE;
    return stzs_launch(frame_rows_kernel, dim3(nblk((long)a->B * a->n)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), *a);
}

extern "C" int stzs_embed(const int32_t* tok, const float* emb, void* y, int B, int T, int D, int64_t ldy,
                          void* stream) {
    if (!tok || !emb || !y) return STZS_EINVAL;
    if (B <= 0 || T <= 0 || D <= 0) return STZS_ESHAPE;
    return stzs_launch(embed_kernel<bf16_t>, dim3(T, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), tok, emb,
                       reinterpret_cast<bf16_t*>(y), B, T, D, (long)ldy);
}

extern "C" int stzs_embed_f32(const int32_t* tok, const float* emb, float* y, int B, int T, int D, int64_t ldy,
                              void* stream) {
    if (!tok || !emb || !y) return STZS_EINVAL;
    if (B <= 0 || T <= 0 || D <= 0) return STZS_ESHAPE;
    return stzs_launch(embed_kernel<float>, dim3(T, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), tok, emb,
                       y, B, T, D, (long)ldy);
}

extern "C" int stzs_embed_lens(const int32_t* tok, const float* emb, void* y, const int32_t* lens, int B, int T,
                               int D, int64_t ldy, int out_dtype, void* stream) {
    if (!tok || !emb || !y || !lens) return STZS_EINVAL;
    if (B <= 0 || T <= 0 || D <= 0) return STZS_ESHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (out_dtype == STZS_BF16)
        return stzs_launch(embed_lens_kernel<bf16_t>, dim3(T, B), dim3(256), 0, s, tok, emb,
                           reinterpret_cast<bf16_t*>(y), lens, B, T, D, (long)ldy);
    else if (out_dtype == STZS_F32)
        return stzs_launch(embed_lens_kernel<float>, dim3(T, B), dim3(256), 0, s, tok, emb,
                           reinterpret_cast<float*>(y), lens, B, T, D, (long)ldy);
    else
        return STZS_EDTYPE;
}

extern "C" int stzs_init(int device) {
    if (hipSetDevice(device) != hipSuccess) return STZS_EHIP;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return STZS_EHIP;
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) return STZS_EINVAL;  // built for CDNA4 only
    return STZS_OK;
}

extern "C" int stzs_version(void) { return 1; }

extern "C" const char* stzs_strerror(int code) {
    switch (code) {
        case STZS_OK: return "ok";
        case STZS_EINVAL: return "STZS_EINVAL: invalid argument (null pointer, enum or alignment)";
        case STZS_ESHAPE: return "STZS_ESHAPE: shape or stride violation";
        case STZS_EDTYPE: return "STZS_EDTYPE: unsupported dtype combination";
        case STZS_EHIP: return "STZS_EHIP: HIP runtime error";
        default: return "unknown stzs error";
    }
}
