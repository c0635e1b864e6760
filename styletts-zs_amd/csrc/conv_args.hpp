// Host-side rules about a stzs_conv_args that more than one file needs: the weight forms of stzs_conv1d (which flag
// bit selects which launcher, and what may not accompany it), the "plain linear" predicate, and the form-independent
// argument validation (stzs_conv_check, csrc/dispatch.hip).  No device code.
#pragma once
#include "common.hpp"

// A 1x1 conv that is a plain GEMM over the B x T rows: one tap, no stride / padding / upsampling, no prologue.  Each
// kernel form adds its own conditions beside its use (no fused statistics, no fp8 row scale, pro_cscale 1, ...).
static inline bool stzs_plain_linear(const stzs_conv_args& a) {
    return a.ks == 1 && a.stride == 1 && a.pad == 0 && a.ups == 0 && a.T_in == a.T_out && a.pro_mode == STZS_PRO_NONE &&
           a.pro_act == STZS_ACT_NONE;
}

// The weight forms, in routing order: the first row whose bit is set in a.flags names the launcher (the last row, bit
// 0, is the generic conv_mfma / gemm_glds path).  `excludes`: flag bits that are an error (STZS_EINVAL) beside it;
// `splitk`: whether the form has a split-K variant; `taps`: whether it reads ks / dil / stride (a ROWS linear does not);
// `t_lens`: whether the form has kernels that honour the ragged frame lengths (stzs_conv_args.t_lens: the generic
// conv_mfma path without STZS_CONV_A_DMA, and the register-direct form's k3 LeakyReLU / identity block convs --
// the precise forms likewise: FRAG32X3's k3 block convs, conv_x3's per-utterance fp32 tiles --
// stzs_conv_check holds the rule common to all, each launcher what is particular to its kernels).
// `t_rows`: whether the form has kernels that honour an utterance's own row count (t_lens with t_lens_rows = 1, the
// ragged decoder: the register-direct form's Snake convs and its polyphase ConvTranspose, the narrow conv_post form;
// on fp32 rows the precise forms' Snake / conv_post convs (FRAG32X3) and conv_x3's convs and ConvTranspose).
// Only the generic path takes prologue statistics from partials (pro_part), and not with STZS_CONV_A_DMA.
struct stzs_conv_form {
    int bit, excludes;
    bool splitk, taps, t_lens, t_rows;
};
constexpr int STZS_CONV_OLD_FORMS = STZS_CONV_W_LANE16 | STZS_CONV_W_NARROW32 | STZS_CONV_W_F32;
constexpr stzs_conv_form STZS_CONV_FORMS[] = {
    {STZS_CONV_W_FRAG32X3, STZS_CONV_OLD_FORMS | STZS_CONV_W_X3 | STZS_CONV_A_DMA | STZS_CONV_W_FRAG32 | STZS_CONV_ROWS |
                               STZS_CONV_UPS_NOISE, false, true, true, true},                      // csrc/mrfx.hip
    {STZS_CONV_W_FRAG32, STZS_CONV_OLD_FORMS | STZS_CONV_A_DMA, false, true, true, true},   // csrc/mrfv.hip, csrc/ups.hip
    {STZS_CONV_ROWS, STZS_CONV_OLD_FORMS | STZS_CONV_W_X3, true, false, false, false},       // csrc/rows.hip
    {STZS_CONV_W_X3, STZS_CONV_OLD_FORMS, false, true, true, true},                          // csrc/convx.hip conv_x3
    {STZS_CONV_W_F32, STZS_CONV_W_LANE16 | STZS_CONV_W_NARROW32, false, true, false, false},       // csrc/convx.hip conv_f32
    {STZS_CONV_W_LANE16, 0, false, true, false, false},                                      // csrc/mrf.hip mrf_conv
    {STZS_CONV_W_NARROW32, 0, false, true, false, true},                                     // csrc/mrf.hip narrow_conv
    {0, 0, true, true, true, false},                                                         // csrc/conv.hip, csrc/gemm.hip
};
// every bit that takes a call off the generic path's conv_mfma kernels (the pair launch and pro_part refuse them)
constexpr int STZS_CONV_NOT_GENERIC = STZS_CONV_OLD_FORMS | STZS_CONV_W_X3 | STZS_CONV_W_FRAG32 | STZS_CONV_W_FRAG32X3 |
                                      STZS_CONV_ROWS | STZS_CONV_A_DMA;

static inline const stzs_conv_form& stzs_conv_form_of(int flags) {
    const stzs_conv_form* f = STZS_CONV_FORMS;
    while (f->bit && !(flags & f->bit)) ++f;
    return *f;
}

// the form-independent validation of one stzs_conv1d problem (before any HIP call): STZS_OK or the first failing
// check's code.  A launcher checks only what is particular to its kernels after it.
int stzs_conv_check(const stzs_conv_args* a);
