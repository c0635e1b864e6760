// stzs_conv1d / stzs_conv1d_group entries (include/stzs.h): the argument checks shared by every conv form
// (stzs_conv_check), then the form's launcher by the table of csrc/conv_args.hpp.  Kept in its own translation unit
// so that adding a kernel form does not rebuild conv.hip.
#include "conv_args.hpp"

int stzs_conv1d_core(const stzs_conv_args* a, void* stream);           // csrc/conv.hip
int stzs_mrfv_conv_launch(const stzs_conv_args& a, hipStream_t s);    // csrc/mrfv.hip
int stzs_rows_gemm_launch(const stzs_conv_args& a, hipStream_t s);    // csrc/rows.hip
int stzs_mrfx_conv_launch(const stzs_conv_args& a, hipStream_t s);    // csrc/mrfx.hip

int stzs_mrfv_trio_launch(const stzs_conv_args* a, hipStream_t s);   // csrc/mrfv.hip
int stzs_conv_pair_launch(const stzs_conv_args* a, hipStream_t s);    // csrc/conv.hip

__attribute__((visibility("hidden"))) int stzs_conv_check(const stzs_conv_args* a) {
    if (!a || !a->x || !a->w || !a->y) return STZS_EINVAL;
    const stzs_conv_form& f = stzs_conv_form_of(a->flags);
    if (a->flags & f.excludes) return STZS_EINVAL;
    if (a->pro_part && (a->flags & STZS_CONV_NOT_GENERIC)) return STZS_EINVAL;  // (the generic conv path only)
    if (a->B <= 0 || a->T_in <= 0 || a->T_out <= 0 || a->Ci <= 0 || a->Co <= 0) return STZS_ESHAPE;
    if (f.taps && (a->ks <= 0 || a->dil <= 0 || a->stride <= 0)) return STZS_ESHAPE;
    if (a->ci_pad < a->Ci || a->co_pad < a->Co) return STZS_ESHAPE;
    // output channels in tiles of 128 (but the polyphase ConvTranspose, csrc/ups.hip, which tiles ups x Co itself)
    if (a->co_pad % 128 && !(f.bit == STZS_CONV_W_FRAG32 && a->ups > 0)) return STZS_ESHAPE;
    // input rows are read as 16-byte vectors of 8 bf16 channels (32-byte ones of fp32: the precise forms' own check)
    if (a->ldx % 8 || a->bsx % 8 || a->ldx < ((a->Ci + 7) / 8) * 8) return STZS_ESHAPE;
    if (!stzs_aligned(a->x, 16) || !stzs_aligned(a->w, 16)) return STZS_EINVAL;
    if (a->pro_mode == STZS_PRO_ADAIN && ((!a->pro_part && (!a->pro_mean || !a->pro_rstd)) || !a->pro_gb)) return STZS_EINVAL;
    if (a->pro_act == STZS_ACT_SNAKE && !a->pro_alpha) return STZS_EINVAL;
    if (a->stat_part && !stzs_aligned(a->stat_part, 8)) return STZS_EINVAL;
    if (a->splitk > 1 && !f.splitk) return STZS_EINVAL;
    if (a->t_lens_rows != 0 && (a->t_lens_rows != 1 || !a->t_lens)) return STZS_EINVAL;
    if (a->t_lens && a->t_lens_rows == 1) {
        // the ragged decoder: t_lens[b] is the utterance's own row count on this launch's input time axis.  A form
        // with such kernels, bf16 rows, stride 1, per-utterance tiles (not a plain linear), no split-K, no pro_part,
        // no multiplier; row for row, or the polyphase ConvTranspose's T_in + 1 GEMM rows (each launcher: the rest).
        // The precise forms (FRAG32X3, X3) take fp32 rows and only those
        const bool x3 = f.bit == STZS_CONV_W_FRAG32X3 || f.bit == STZS_CONV_W_X3;
        if (!f.t_rows || (a->flags & STZS_CONV_A_DMA) || a->stride != 1 || a->splitk > 1 || a->pro_part ||
            stzs_plain_linear(*a) || a->in_dtype != (x3 ? STZS_F32 : STZS_BF16) || a->t_lens_mul < 0 || a->t_lens_mul > 1 ||
            (a->ups > 0 ? a->T_out != a->T_in + 1 : (a->ups != 0 || a->T_out != a->T_in)) || !stzs_aligned(a->t_lens, 4))
            return STZS_EINVAL;
    } else if (a->t_lens) {
        // ragged frame batch: a form with length-aware kernels (the generic one: not its LDS-DMA GEMM), row for row
        // (stride 1, T_out == T_in, no ConvTranspose), per-utterance tiles (not a plain linear), no split-K, the
        // prologue statistics finalised (no pro_part)
        if (!f.t_lens || (a->flags & STZS_CONV_A_DMA) || a->stride != 1 || a->T_out != a->T_in || a->ups != 0 ||
            a->splitk > 1 || a->pro_part || stzs_plain_linear(*a) || a->in_dtype == STZS_F8 || a->t_lens_mul < 0 ||
            a->t_lens_mul > 2 || !stzs_aligned(a->t_lens, 4))
            return STZS_EINVAL;
    }
    return STZS_OK;
}

extern "C" int stzs_conv1d_group(const stzs_conv_args* a, int n, void* stream) {
    if (!a || n < 1 || n > 3) return STZS_EINVAL;
    const auto trio_member = [](const stzs_conv_args& p) {  // a valid FRAG32 conv (not the ConvTranspose form)
        return stzs_conv_form_of(p.flags).bit == STZS_CONV_W_FRAG32 && p.ups <= 0 && !p.t_lens &&
               stzs_conv_check(&p) == STZS_OK;  // (with t_lens: one stzs_conv1d each, refused or honoured there)
    };
    if (n == 3 && trio_member(a[0]) && trio_member(a[1]) && trio_member(a[2])) {
        const int rc = stzs_mrfv_trio_launch(a, reinterpret_cast<hipStream_t>(stream));
        if (rc == STZS_OK) return 1;
        if (rc != STZS_ESHAPE) return rc;
    }
    if (n == 2 && !a[0].pro_part == !a[1].pro_part && !a[0].t_lens && !a[1].t_lens) {  // (pro_part: both or neither, as the body reads it uniformly)
        const int rc = stzs_conv_pair_launch(a, reinterpret_cast<hipStream_t>(stream));
        if (rc == STZS_OK) return 1;
        if (rc != STZS_ESHAPE) return rc;
    }
    for (int i = 0; i < n; ++i) {  // one after the other (the same results)
        const int rc = stzs_conv1d(&a[i], stream);
        if (rc != STZS_OK) return rc;
    }
    return n;
}

extern "C" int stzs_conv1d(const stzs_conv_args* a, void* stream) {
    const int rc = stzs_conv_check(a);
    if (rc != STZS_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (stzs_conv_form_of(a->flags).bit) {
        case STZS_CONV_W_FRAG32X3: return stzs_mrfx_conv_launch(*a, s);  // the precise register-direct form
        case STZS_CONV_W_FRAG32: return stzs_mrfv_conv_launch(*a, s);
        case STZS_CONV_ROWS: return stzs_rows_gemm_launch(*a, s);
        default: return stzs_conv1d_core(a, stream);
    }
}
