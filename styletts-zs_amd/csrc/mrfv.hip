// The MRF conv, register-direct weight form: the launcher (stzs_mrfv_conv_launch) and the
// multi-chunk instances -- the wide stage-0 forms, the decoder / predictor AdaIN-block k3 convs and the length-aware
// (RAG) instances of both: the block forms' for ragged frame batches, the Snake forms' for the ragged decoder
// (stzs_conv_args.t_lens, t_lens_rows 0 / 1).  The kernel template
// and its design notes: csrc/mrfv_kernel.hpp; the single-chunk stage-1 instances: csrc/mrfv_n1.hip.
#include "mrfv_kernel.hpp"

namespace {

template <int PACT, bool HR, bool HA>
void (*pick(int ks, bool one, bool al, bool wide, bool t64))(stzs_conv_args) {
    if (wide) return al ? pick_ks<PACT, HR, HA, 0, true, 2>(ks) : pick_ks<PACT, HR, HA, 0, false, 2>(ks);
    static_assert(PACT == STZS_ACT_SNAKE, "the single-chunk forms are the Snake (MRF) convs");
    if (one) return stzs_mrfv_pick_n1(ks, HR, HA, al, t64);  // (csrc/mrfv_n1.hip)
    if (t64)  // (64-row tiles: the Snake forms of small grids)
        return al ? pick_ks<PACT, HR, HA, 0, true, 1, 64>(ks) : pick_ks<PACT, HR, HA, 0, false, 1, 64>(ks);
    return al ? pick_ks<PACT, HR, HA, 0, true>(ks) : pick_ks<PACT, HR, HA, 0, false>(ks);
}

}  // namespace

int stzs_ups_conv_launch(const stzs_conv_args& a, hipStream_t s);   // csrc/ups.hip (polyphase ConvTranspose)

namespace {

// the launcher's own conditions (beyond stzs_conv_check, csrc/dispatch.hip): bf16 rows of 16-byte vectors in and out,
// 128-channel chunks, the staged rows of a tile within its capacity
int mrfv_shape(const stzs_conv_args& a) {
    if (a.in_dtype == STZS_F8 || a.x_scale) return STZS_EDTYPE;
    if (!stzs_aligned(a.y, 16)) return STZS_EINVAL;
    if (a.ups > 0) return STZS_OK;  // (the ConvTranspose form: csrc/ups.hip checks the rest)
    // the ragged decoder (t_lens_rows 1): the Snake convs only, with one of the generator's four epilogue combinations
    // (pick_rag, csrc/mrfv_kernel.hpp) -- the block forms keep the §2d rule below
    if (a.t_lens && a.t_lens_rows == 1 &&
        (a.pro_act != STZS_ACT_SNAKE || (a.ks != 3 && a.ks != 7 && a.ks != 11) || (!a.res && (a.acc_in || a.alpha != 1.f))))
        return STZS_EINVAL;
    const int rows_in = 128 + (a.ks - 1) * a.dil;
    if (a.stride != 1 || a.cic != 128 || a.ci_pad % 128 || a.Co % 8 || rows_in > 16 * sb_rows(a.ks) ||
        a.in_dtype != STZS_BF16 || a.out_dtype != STZS_BF16 || a.gate || a.epi_act != STZS_ACT_NONE || a.ups ||
        a.refl || a.ldy % 8 || a.bsy % 8 || (a.res && (a.ldr % 8 || a.bsr % 8 || a.res_tdiv <= 0)) ||
        (a.acc_in && (a.lda % 8 || a.bsa % 8)) || (a.stat_part && a.stat_ld < a.Co))
        return STZS_ESHAPE;
    if (a.pro_act == STZS_ACT_SNAKE && a.res && a.res_tdiv != 1) return STZS_ESHAPE;  // (TD1 in the kernel)
    // ragged frame batch (t_lens): the k3 LeakyReLU / identity block convs only (stzs_conv_check: the rest of the rule)
    if (a.t_lens && a.t_lens_rows == 0 &&
        (a.ks != 3 || a.acc_in || (a.pro_act != STZS_ACT_LEAKY && a.pro_act != STZS_ACT_NONE)))
        return STZS_EINVAL;
    return STZS_OK;
}

// The tile choice of a launch, computed once (every form is bit-identical, so the choice never changes a result).
// Snake forms: the wide form for multi-chunk convs whose wide grid still gives every CU two workgroups (at batch 1 a
// stage-0 conv has 32 row tiles: the narrow form's 64 workgroups finish sooner); else 64-row tiles where the narrow
// 128-row grid would not give every CU two workgroups (batch 1: a stage-1 conv is 188 tiles, a stage-0 conv 64).
// AdaIN-block convs: (r05) the wide form where the wide grid gives every CU two workgroups (a decoder conv at 64
// utterances: 512 wide tiles): each 9-chunk input row staged once per 256 output channels instead of per 128 --
// 111 -> 88 us per 1024-channel decoder conv at B = 64; at 32 utterances (256 wide tiles) the narrow form is as
// fast (56.4 vs 57.5 us), so it stays there (`tools/blk_probe.py` FRAG32=1).  64-row tiles for the narrow block convs
// below 4 128-row tiles per CU (a decoder conv at 32 utterances: 512 tiles; 57.1 -> 55.2 us, the predictor's
// 256-channel convs 24.4 -> 21.8): more, shorter workgroups per CU hide more of each input chunk's staging latency;
// STZS_MRFV_T64_BLK=N sets that threshold for the k3 convs (0: off).  (r06) the blocks' 1x1 shortcut convs (1090 ->
// 1024 at the decoder) likewise: the block convs' data movement with one tap -- as a FLAT LDS-DMA GEMM they ran at 0.11
// of their roofline, streaming A and B tiles through LDS.
// STZS_CONV_MRFV_NARROW refuses the wide form, STZS_CONV_MRFV_T128 keeps 128-row tiles.
void mrfv_tiles(const stzs_conv_args& a, bool& wide, bool& t64) {
    static const int t64_blk = [] {
        const char* e = getenv("STZS_MRFV_T64_BLK");
        return e ? atoi(e) : 4;
    }();
    const bool snake = a.pro_act == STZS_ACT_SNAKE;
    const long cu = stzs_cu_count();
    const long wide_tiles = (long)a.B * ((a.T_out + 127) / 128) * (a.co_pad / (2 * BCO));
    const long tiles128 = (long)a.B * ((a.T_out + 127) / 128) * (a.co_pad / BCO);
    const int rows64 = 64 + (a.ks - 1) * a.dil;
    wide = a.ci_pad > 128 && a.co_pad % (2 * BCO) == 0 && wide_tiles >= (snake ? 512 : 2 * cu) &&
           !(a.flags & STZS_CONV_MRFV_NARROW);
    t64 = !wide && tiles128 < (snake ? 2 : a.ks == 1 ? 4 : t64_blk) * cu && !(a.flags & STZS_CONV_MRFV_T128) &&
          (!snake || rows64 <= 16 * (a.ks == 3 ? sb_rows64(3) : a.ks == 7 ? sb_rows64(7) : sb_rows64(11)));
}

}  // namespace

// (r06) the k3 / k7 / k11 convs of one MRF layer in one launch (mrfv_trio, csrc/mrfv_kernel.hpp): STZS_ESHAPE unless
// a[0..2] have ks 3, 7, 11, the Snake prologue, no accumulate input, alpha 1, the same B / T_out / Ci / Co / padding
// and residual-ness, and each would take the narrow 64-row form on its own (the small grids of batch 1).  The caller
// (stzs_conv1d_group) has run stzs_conv1d's argument checks on each.
__attribute__((visibility("hidden"))) int stzs_mrfv_trio_launch(const stzs_conv_args* a, hipStream_t s) {
    static const int KS[3] = {3, 7, 11};
    size_t lds = 0;
    for (int i = 0; i < 3; ++i) {
        const stzs_conv_args& b = a[i];
        bool wide, t64;
        mrfv_tiles(b, wide, t64);
        if (mrfv_shape(b) != STZS_OK || b.t_lens || b.ks != KS[i] || b.pro_act != STZS_ACT_SNAKE || b.acc_in || b.alpha != 1.f || !t64 ||
            b.B != a[0].B || b.T_out != a[0].T_out || b.Ci != a[0].Ci || b.Co != a[0].Co || b.ci_pad != a[0].ci_pad ||
            b.co_pad != a[0].co_pad || (b.res != nullptr) != (a[0].res != nullptr))
            return STZS_ESHAPE;
        const size_t l = mrfv_lds(64 + (b.ks - 1) * b.dil);
        lds = l > lds ? l : lds;
    }
    const bool R = a[0].res != nullptr;
    void (*k)(stzs_conv_args, stzs_conv_args, stzs_conv_args) =
        a[0].ci_pad == 128 ? stzs_mrfv_trio_pick_n1(R) : (R ? mrfv_trio<true, 0, 64> : mrfv_trio<false, 0, 64>);
    dim3 grid((unsigned)a[0].B * (unsigned)((a[0].T_out + 63) / 64), a[0].co_pad / BCO, 3);
    return stzs_launch(k, grid, dim3(NTH), lds, s, a[0], a[1], a[2]);
}

// internal entry used by stzs_conv1d for STZS_CONV_W_FRAG32 weights
__attribute__((visibility("hidden"))) int stzs_mrfv_conv_launch(const stzs_conv_args& a, hipStream_t s) {
    {
        const int rc = mrfv_shape(a);
        if (rc != STZS_OK) return rc;
    }
    if (a.ups > 0) return stzs_ups_conv_launch(a, s);
    const bool R = a.res != nullptr, A = a.acc_in != nullptr;
    bool wide, t64;
    mrfv_tiles(a, wide, t64);
    mrfv_kfn k = nullptr;
    if (a.pro_act == STZS_ACT_SNAKE && a.t_lens) {
        // (mrfv_shape: t_lens_rows 1) the ragged decoder's instances, all at 128-row tiles: single-chunk, wide where the
        // uniform launch would be wide, else narrow -- every tile form is bit-identical
        t64 = false;
        const bool al = a.alpha != 1.f;
        k = a.ci_pad == 128 ? stzs_mrfv_pick_n1_rag(a.ks, R, A, al)
                            : wide ? pick_rag<0, 2>(a.ks, R, A, al) : pick_rag<0, 1>(a.ks, R, A, al);
    } else if (a.pro_act == STZS_ACT_SNAKE) {
        const bool one = a.ci_pad == 128;
        const bool al = a.alpha != 1.f;
        k = R ? (A ? pick<STZS_ACT_SNAKE, true, true>(a.ks, one, al, wide, t64) : pick<STZS_ACT_SNAKE, true, false>(a.ks, one, al, wide, t64))
              : (A ? pick<STZS_ACT_SNAKE, false, true>(a.ks, one, al, wide, t64) : pick<STZS_ACT_SNAKE, false, false>(a.ks, one, al, wide, t64));
    } else if (!A && a.ks == 1 && a.pro_act == STZS_ACT_NONE && a.pro_mode == STZS_PRO_NONE && !a.stat_part) {
        // the AdaIN blocks' 1x1 shortcut convs
        k = wide ? (R ? mrfv_conv<STZS_ACT_NONE, true, false, 1, 0, true, 2> : mrfv_conv<STZS_ACT_NONE, false, false, 1, 0, true, 2>)
          : t64 ? (R ? mrfv_conv<STZS_ACT_NONE, true, false, 1, 0, true, 1, 64> : mrfv_conv<STZS_ACT_NONE, false, false, 1, 0, true, 1, 64>)
                 : (R ? mrfv_conv<STZS_ACT_NONE, true, false, 1, 0, true> : mrfv_conv<STZS_ACT_NONE, false, false, 1, 0, true>);
    } else if (a.t_lens) {  // (mrfv_shape: k3, LeakyReLU / identity, no accumulate input) the lengths' own instances
        if (a.pro_act == STZS_ACT_LEAKY)
            k = wide ? (R ? mrfv_conv<STZS_ACT_LEAKY, true, false, 3, 0, true, 2, 128, true> : mrfv_conv<STZS_ACT_LEAKY, false, false, 3, 0, true, 2, 128, true>)
              : t64 ? (R ? mrfv_conv<STZS_ACT_LEAKY, true, false, 3, 0, true, 1, 64, true> : mrfv_conv<STZS_ACT_LEAKY, false, false, 3, 0, true, 1, 64, true>)
                     : (R ? mrfv_conv<STZS_ACT_LEAKY, true, false, 3, 0, true, 1, 128, true> : mrfv_conv<STZS_ACT_LEAKY, false, false, 3, 0, true, 1, 128, true>);
        else
            k = wide ? (R ? mrfv_conv<STZS_ACT_NONE, true, false, 3, 0, true, 2, 128, true> : mrfv_conv<STZS_ACT_NONE, false, false, 3, 0, true, 2, 128, true>)
              : t64 ? (R ? mrfv_conv<STZS_ACT_NONE, true, false, 3, 0, true, 1, 64, true> : mrfv_conv<STZS_ACT_NONE, false, false, 3, 0, true, 1, 64, true>)
                     : (R ? mrfv_conv<STZS_ACT_NONE, true, false, 3, 0, true, 1, 128, true> : mrfv_conv<STZS_ACT_NONE, false, false, 3, 0, true, 1, 128, true>);
    } else if (!A && a.ks == 3) {  // the AdaIN residual blocks of the decoder / prosody predictor
        if (a.pro_act == STZS_ACT_LEAKY)
            k = wide ? (R ? mrfv_conv<STZS_ACT_LEAKY, true, false, 3, 0, true, 2> : mrfv_conv<STZS_ACT_LEAKY, false, false, 3, 0, true, 2>)
              : t64 ? (R ? mrfv_conv<STZS_ACT_LEAKY, true, false, 3, 0, true, 1, 64> : mrfv_conv<STZS_ACT_LEAKY, false, false, 3, 0, true, 1, 64>)
                     : (R ? mrfv_conv<STZS_ACT_LEAKY, true, false, 3, 0, true> : mrfv_conv<STZS_ACT_LEAKY, false, false, 3, 0, true>);
        else if (a.pro_act == STZS_ACT_NONE)
            k = wide ? (R ? mrfv_conv<STZS_ACT_NONE, true, false, 3, 0, true, 2> : mrfv_conv<STZS_ACT_NONE, false, false, 3, 0, true, 2>)
              : t64 ? (R ? mrfv_conv<STZS_ACT_NONE, true, false, 3, 0, true, 1, 64> : mrfv_conv<STZS_ACT_NONE, false, false, 3, 0, true, 1, 64>)
                     : (R ? mrfv_conv<STZS_ACT_NONE, true, false, 3, 0, true> : mrfv_conv<STZS_ACT_NONE, false, false, 3, 0, true>);
    }
    if (!k) return STZS_ESHAPE;
    const int BTk = t64 ? 64 : 128;
    dim3 grid((unsigned)a.B * (unsigned)((a.T_out + BTk - 1) / BTk), a.co_pad / (wide ? 2 * BCO : BCO));
    return stzs_launch(k, grid, dim3(NTH), mrfv_lds(BTk + (a.ks - 1) * a.dil), s, a);
}
