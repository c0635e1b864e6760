"""The case table of tests/test_gpu_ragged_precise_kernels.py as data (no device, no library): every distinct launch
shape the GPU test makes with lengths, and its refusals.  tools/dispatch_trace.py --ragged-precise-cases runs the table
through the real host dispatch with the recording runtime stand-in; tests/test_ragged_precise_host.py checks that trace.

A case is a dict: form ("fx3": STZS_CONV_W_FRAG32X3, "x3": STZS_CONV_W_X3), B, T, Ci, Co, ks, dil, act ("snake" |
"leaky" | "none"), adain, res, tdiv, acc, stat, alpha, mode (t_lens_rows), mul (t_lens_mul), ups, refl, and for a
refusal `over` (fields set last) with want = -1 (STZS_EINVAL)."""
import math

# the 64-row statistics chunk edge, the 128-row tile edge, a row shorter than the k11 d5 halo (25 rows a side)
LENS = {"a": [200, 2, 64, 129], "b": [199, 65, 128, 63]}
T_CONV = 200
# (7, 5): the 158-row 128-row tile; (11, 3) / (11, 5): the 64-row tiles
KD = [(3, 1), (3, 5), (7, 3), (7, 5), (11, 1), (11, 3), (11, 5)]
# the generator's four epilogue combinations (csrc/mrfv_kernel.hpp pick_rag)
EPI = {"plain": dict(), "res": dict(res=True), "res_alpha": dict(res=True, alpha=1 / 3),
       "res_acc_alpha": dict(res=True, acc=True, alpha=1 / 3)}
BLK_SHAPES = {"T130": (130, [130, 65, 128, 63]), "T37": (37, [37, 9, 20, 3]), "T12": (12, [12, 5, 9, 1])}
X3_SNAKE_KD = [(3, 1), (7, 3), (11, 5)]


def _case(label, form, Ci, Co, ks, dil, act, T, mode, **kw):
    d = dict(label=label, form=form, B=4, T=T, Ci=Ci, Co=Co, ks=ks, dil=dil, act=act, adain=act != "none", res=False,
             tdiv=1, acc=False, stat=False, alpha=1.0, mode=mode, mul=0, ups=0, refl=0, want=0, over={})
    d.update(kw)
    return d


def accepted():
    """-> the launches with lengths the GPU test makes (one per distinct shape; the lengths are device data)"""
    out = []
    for Ci in (128, 256):
        for ks, dil in KD:
            for e, kw in EPI.items():
                out.append(_case(f"mrfx.snake Ci{Ci} k{ks}d{dil} {e}", "fx3", Ci, 128, ks, dil, "snake", T_CONV, 1, stat=True, **kw))
    for ks, dil in X3_SNAKE_KD:
        for e in ("plain", "res_acc_alpha"):
            out.append(_case(f"x3.snake k{ks}d{dil} {e}", "x3", 128, 128, ks, dil, "snake", T_CONV, 1, stat=True, **EPI[e]))
    out.append(_case("mrfx.conv_post", "fx3", 128, 22, 7, 1, "leaky", T_CONV, 1, adain=False))
    for name, (T, _) in BLK_SHAPES.items():
        for mul in (1, 2):
            for act in ("leaky", "none"):
                for res, tdiv in ((False, 1), (True, 1), (True, 2)):
                    out.append(_case(f"mrfx.blk {name} {act} res{int(res)} tdiv{tdiv} mul{mul}", "fx3", 256, 128, 3, 1, act,
                                     T * mul, 0, mul=mul, res=res, tdiv=tdiv, stat=True, alpha=1 / math.sqrt(2.0)))
            out.append(_case(f"x3.blk {name} leaky mul{mul}", "x3", 48, 40, 3, 1, "leaky", T * mul, 0, mul=mul, res=True,
                             tdiv=2, stat=True, alpha=1 / math.sqrt(2.0)))
            out.append(_case(f"x3.blk {name} none mul{mul}", "x3", 48, 40, 3, 1, "none", T * mul, 0, mul=mul, stat=True,
                             alpha=1 / math.sqrt(2.0)))
    for refl in (0, 1):
        out.append(_case(f"x3.ups r5 refl{refl}", "x3", 256, 128, 2, 1, "leaky", T_CONV, 1, adain=False, res=True, ups=5,
                         refl=refl))
    return out


def refused():
    """-> the calls with lengths that return STZS_EINVAL before any runtime call"""
    BF16 = 1
    out = []
    for form in ("fx3", "x3"):
        for mode in (0, 1):
            out.append(_case(f"{form}.flat linear mode{mode}", form, 128, 128, 1, 1, "none", 40, mode, want=-1))
        out.append(_case(f"{form}.snake bf16 rows", form, 128, 128, 3, 1, "snake", 40, 1, want=-1, over=dict(in_dtype=BF16)))
        out.append(_case(f"{form}.blk stride 2", form, 256, 128, 3, 1, "leaky", 40, 0, want=-1, over=dict(stride=2, T_out=20)))
        out.append(_case(f"{form}.snake rows 1 mul 2", form, 128, 128, 3, 1, "snake", 40, 1, mul=2, want=-1))
    out.append(_case("fx3.snake acc no res", "fx3", 128, 128, 3, 1, "snake", 40, 1, acc=True, want=-1))
    out.append(_case("fx3.snake rows 0", "fx3", 128, 128, 3, 1, "snake", 40, 0, want=-1))
    out.append(_case("fx3.k7 leaky rows 0", "fx3", 128, 128, 7, 1, "leaky", 40, 0, want=-1))
    return out
