"""Kernel-level dispatch trace (the CPU counterpart of tools/launch_trace.py one level down): which kernel instance,
grid, block and LDS size every library call launches -- recorded WITHOUT a device.  The objects of a library build are
linked with the recording runtime stand-in tools/hip_record/hip_record.cpp into libstzs_trace.so (g++, --no-undefined,
-Bsymbolic: the library's runtime references bind to the stand-in even beside a loaded HIP runtime), and the real host
dispatch runs with fixed fake pointers: nothing is dereferenced, nothing launched.  Two builds whose traces are equal
route every traced call to the same kernels with the same launch geometry: the check for a host-side refactor.

    python tools/dispatch_trace.py --synth tiny --out a.txt          # the eight cases of tools/launch_trace.py
    python tools/dispatch_trace.py --sweep --out b.txt               # generated argument structs, valid and broken
    python tools/dispatch_trace.py --objects OTHER/build --lib /tmp/o.so --sweep --out c.txt     # another build
    python tools/dispatch_trace.py --coverage a.txt b.txt            # registered conv-family kernels never launched
    python tools/dispatch_trace.py --linear-cases --out d.txt        # the identity-probe table of the linears' GPU test
    python tools/dispatch_trace.py --precise-cases --out e.txt       # every launch of the precise convs' GPU test
    python tools/dispatch_trace.py --ragged-precise-cases --out f.txt   # the precise convs with per-row lengths (§2i)

Trace lines (hip_record.cpp): "L kernel gx gy gz bx by bz lds", "A kernel attribute value" (hipFuncSetAttribute),
"C memcpy|memset bytes", "M text" (this driver's markers: "case NAME" before a synthesis case, "call LABEL" / "rc N"
around a sweep call).  The launcher's environment switches (STZS_ROWS16_WPG, STZS_GEMM_TILE, STZS_UPS_BT,
STZS_MRFV_T64_BLK) are read once per process: set them in the environment of a run of this tool.
The trace library is only ever used with device "cpu"; nothing on a GPU path loads it.
"""
import argparse
import ctypes as C
import hashlib
import itertools
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "styletts-zs_amd")
OBJECTS = os.path.join(PKG, "build")
STANDIN = os.path.join(ROOT, "tools", "hip_record", "hip_record.cpp")
CONV_OBJECTS = ("mrf", "mrfv", "mrfv_n1", "mrfx", "conv", "convx", "gemm", "rows", "lnrows", "ups")
sys.path[:0] = [ROOT, PKG]


def objects_of(objdir):
    return sorted(os.path.join(objdir, f) for f in os.listdir(objdir) if f.endswith(".o")) if os.path.isdir(objdir) else []


def build_trace_lib(objdir=OBJECTS, lib=None):
    """link objdir/*.o with the stand-in -> lib (default objdir/libstzs_trace.so); relinked only when out of date"""
    lib = lib or os.path.join(objdir, "libstzs_trace.so")
    objs = objects_of(objdir)
    if not objs:
        raise RuntimeError(f"no objects in {objdir}: run styletts-zs_amd/build.py")
    if os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(p) for p in objs + [STANDIN]):
        return lib
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-shared", "-fPIC", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", STANDIN] + objs + \
          ["-Wl,--no-undefined", "-Wl,-Bsymbolic", "-o", lib + ".tmp"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr}")
    os.replace(lib + ".tmp", lib)
    return lib


def _load(lib, out):
    """point the package at the trace library, the stand-in at `out` (both before the first call)"""
    if os.path.exists(out):
        os.remove(out)
    os.environ["HIP_RECORD_OUT"] = out
    from stzs import _lib
    _lib.LIB_PATH, _lib._lib = lib, None
    L = _lib.load()
    L.hip_record_mark.argtypes = [C.c_char_p]
    L.hip_record_mark.restype = None
    return L


def parse(path):
    """-> [[kind ("case" | "call"), marker text, return code or None, [trace line, ...]]], one entry per marker"""
    out = []
    for line in open(path).read().splitlines():
        if line.startswith("M case ") or line.startswith("M call "):
            out.append([line[2:6], line[7:], None, []])
        elif line.startswith("M rc "):
            out[-1][2] = int(line[5:])
        elif out:
            out[-1][3].append(line)
    return out


def by_case(entries):
    """{case: (library calls that launched, counting a group call as its return value; kernels; trace lines)}"""
    out, cur = {}, None
    for kind, text, rc, lines in entries:
        if kind == "case":
            cur = out[text] = [0, 0, []]
        elif cur is not None:
            n = sum(ln.startswith("L ") for ln in lines)
            cur[0] += (rc if text.startswith("stzs_conv1d_group") else 1) if n else 0
            cur[1] += n
            cur[2] += [f"M call {text}"] + lines + [f"M rc {rc}"]
    return out


# ---- mode (a): whole syntheses ------------------------------------------------------------------------------------
class _Marking:
    """the loaded library with a "call NAME" / "rc N" marker pair around every stzs_* call"""

    def __init__(self, L):
        self._L = L

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if not name.startswith("stzs_"):
            return f

        def call(*args):
            self._L.hip_record_mark(f"call {name}".encode())
            rc = f(*args)
            self._L.hip_record_mark(f"rc {rc if isinstance(rc, int) else 0}".encode())
            return rc
        return call


def synth(spec, lib, out):
    L = _load(lib, out)
    import launch_trace
    from stzs import _lib
    _lib._lib = _Marking(L)
    res = launch_trace.run_cases(spec, record=False, on_case=lambda n: L.hip_record_mark(f"case {n}".encode()))
    cases = by_case(parse(out))
    for name, _, launches in res:
        counted, kernels, lines = cases[name]
        print(f"{name:15s} engine.launches={launches} launching_calls={counted} kernels={kernels} "
              f"sha256={hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")


# ---- mode (b): the sweep ------------------------------------------------------------------------------------------
F32, BF16, I32, F8 = 0, 1, 2, 3
NONE, LEAKY, SNAKE, GELU, SILU = 0, 1, 2, 3, 4
LANE16, NARROW32, WF32, LINEAR_IDS, FRAG32, X3, ROWS, UPS_NOISE = 16, 32, 64, 128, 256, 1024, 2048, 4096
A_DMA, MRFV_NARROW, FRAG32X3, MRFV_T128, RING, SK_TICKET = 8, 8192, 16384, 32768, 65536, 131072  # include/stzs.h
PTRS = ("x", "w", "bias", "y", "res", "acc_in", "gate", "pro_mean", "pro_rstd", "pro_gb", "pro_alpha", "stat_part",
        "x_scale", "w_scale", "splitk_ws", "splitk_ctr", "pro_part", "t_lens")
PTR = {n: 0x10000000 * (i + 1) for i, n in enumerate(PTRS)}  # fixed, 64-byte aligned, never dereferenced


def rup(v, m):
    return (v + m - 1) // m * m


def conv(B=2, T=100, Ci=128, Co=128, ks=1, dil=1, cic=32, flags=0, ind=BF16, outd=BF16, res=False, acc=False,
         gate=False, pro_act=NONE, adain=False, stat=False, splitk=0, alpha=1.0, ups=0, epi_act=NONE, **over):
    """one valid-by-construction stzs_conv_args as a dict of fields ("same" padding; ups > 0: the ConvTranspose
    geometry); `over` sets fields directly, last"""
    d = dict(x=PTR["x"], w=PTR["w"], bias=PTR["bias"], y=PTR["y"], B=B, T_in=T, T_out=T, Ci=Ci, Co=Co, ks=ks, dil=dil,
             stride=1, pad=dil * (ks - 1) // 2, cic=cic, ci_pad=rup(Ci, cic), co_pad=rup(max(Co, ups * Co), 128),
             flags=flags, in_dtype=ind, out_dtype=outd, pro_act=pro_act, epi_act=epi_act, alpha=alpha, beta=1.0,
             pro_cscale=1.0, pro_slope=0.1, epi_slope=0.1, res_tdiv=1, ups=ups, splitk=splitk)
    if ups > 0:
        d.update(ks=2, pad=1, dil=1, T_out=T + 1, T_final=T * ups)
    ncol = max(Co, ups * Co)
    d["ldx"], d["ldy"] = d["ci_pad"], rup(ncol, 8)
    d["bsx"], d["bsy"] = T * d["ldx"], d["T_out"] * max(ups, 1) * d["ldy"]
    if res:
        d.update(res=PTR["res"], ldr=d["ldy"], bsr=d["bsy"])
    if acc:
        d.update(acc_in=PTR["acc_in"], lda=d["ldy"], bsa=d["bsy"])
    if gate:
        d.update(gate=PTR["gate"], gate_bs=d["co_pad"])
    if pro_act == SNAKE:
        d["pro_alpha"] = PTR["pro_alpha"]
    if adain:
        d.update(pro_mode=1, pro_mean=PTR["pro_mean"], pro_rstd=PTR["pro_rstd"], pro_gb=PTR["pro_gb"],
                 stat_bs=rup(Ci, 8), gb_bs=2 * Ci, gb_beta_off=Ci)
    if stat:
        d.update(stat_part=PTR["stat_part"], stat_ld=rup(Co, 8))
    if splitk > 1:
        d.update(splitk_ws=PTR["splitk_ws"], splitk_ctr=PTR["splitk_ctr"])
    if ind == F8:
        d.update(x_scale=PTR["x_scale"], w_scale=PTR["w_scale"])
    d.update(over)
    return d


def rowln(rows, width, ind=F32, **over):
    Cn = width
    d = dict(x=PTR["x"], y=0, G=PTR["pro_gb"], Bt=PTR["pro_mean"], ldx=Cn, ldy=Cn, gs=Cn, bs=Cn, R=rows, C=Cn, gdiv=1,
             in_dtype=ind, out_dtype=BF16, act=NONE, gadd=1.0, eps=1e-5)
    d.update(over)
    return d


def mutants(d):
    """single-defect (single-field, or one field with the fields that give it meaning) variants of a valid struct"""
    m = []
    for p in ("x", "w", "y"):
        m += [(f"{p}=NULL", {p: 0}), (f"{p}+4", {p: d[p] + 4}), (f"{p}+16", {p: d[p] + 16})]
    for f in ("B", "T_in", "T_out", "Ci", "Co", "ks", "dil", "stride"):
        m += [(f"{f}=0", {f: 0}), (f"{f}=-1", {f: -1})]
    m += [("ci_pad<Ci", {"ci_pad": d["Ci"] - 8}), ("co_pad<Co", {"co_pad": d["Co"] - 8}), ("co_pad+64", {"co_pad": d["co_pad"] + 64}),
          ("ci_pad+16", {"ci_pad": d["ci_pad"] + 16}), ("cic=48", {"cic": 48}), ("cic=0", {"cic": 0})]
    m += [(f"cic={c}", {"cic": c}) for c in (32, 64, 128) if c != d["cic"]]
    for f in ("ldx", "bsx", "ldy", "bsy", "ldr", "bsr", "lda", "bsa"):
        m.append((f"{f}+4", {f: d.get(f, 0) + 4}))
    m += [("ldx=8", {"ldx": 8}), ("adain:no pointers", {"pro_mode": 1}),
          ("adain:no gb", {"pro_mode": 1, "pro_mean": PTR["pro_mean"], "pro_rstd": PTR["pro_rstd"]}),
          ("adain:no rstd", {"pro_mode": 1, "pro_mean": PTR["pro_mean"], "pro_gb": PTR["pro_gb"]}),
          ("pro_mode=2", {"pro_mode": 2}), ("pro_act=GELU", {"pro_act": GELU}), ("pro_act=7", {"pro_act": 7}),
          ("snake:no alpha", {"pro_act": SNAKE, "pro_alpha": 0}), ("pro_act=LEAKY", {"pro_act": LEAKY}),
          ("stat_part+4", {"stat_part": PTR["stat_part"] + 4, "stat_ld": rup(d["Co"], 8)}),
          ("stat_part:ld 0", {"stat_part": PTR["stat_part"], "stat_ld": 0}),
          ("stat_part", {"stat_part": PTR["stat_part"], "stat_ld": rup(d["Co"], 8)}),
          ("pro_part", {"pro_part": PTR["pro_part"], "pro_nch": 2, "pro_T": d["T_in"], "pro_ld": rup(d["Ci"], 8), "pro_mode": 1,
                        "pro_gb": PTR["pro_gb"]}),
          ("pro_part:nch 9", {"pro_part": PTR["pro_part"], "pro_nch": 9, "pro_T": d["T_in"], "pro_ld": rup(d["Ci"], 8)}),
          ("splitk:no ws", {"splitk": 2, "splitk_ws": 0, "splitk_ctr": PTR["splitk_ctr"]}),
          ("splitk:ws+8", {"splitk": 2, "splitk_ws": PTR["splitk_ws"] + 8, "splitk_ctr": PTR["splitk_ctr"]}),
          ("splitk:ctr+2", {"splitk": 2, "splitk_ws": PTR["splitk_ws"], "splitk_ctr": PTR["splitk_ctr"] + 2}),
          ("splitk=2", {"splitk": 2, "splitk_ws": PTR["splitk_ws"], "splitk_ctr": PTR["splitk_ctr"]}),
          ("splitk=3", {"splitk": 3, "splitk_ws": PTR["splitk_ws"], "splitk_ctr": PTR["splitk_ctr"]}),
          ("splitk=32", {"splitk": 32, "splitk_ws": PTR["splitk_ws"], "splitk_ctr": PTR["splitk_ctr"]}),
          ("res:tdiv 0", {"res": PTR["res"], "ldr": d["ldy"], "bsr": d["bsy"], "res_tdiv": 0}),
          ("res:tdiv 2", {"res": PTR["res"], "ldr": d["ldy"], "bsr": d["bsy"], "res_tdiv": 2}),
          ("res+16", {"res": PTR["res"] + 16, "ldr": d["ldy"], "bsr": d["bsy"]}),
          ("acc_in+16", {"acc_in": PTR["acc_in"] + 16, "lda": d["ldy"], "bsa": d["bsy"]}),
          ("gate", {"gate": PTR["gate"]}), ("x_scale", {"x_scale": PTR["x_scale"]}), ("refl=1", {"refl": 1, "T_final": 1}),
          ("ups=2", {"ups": 2}), ("ups=0", {"ups": 0}), ("epi_act=LEAKY", {"epi_act": LEAKY}), ("epi_act=GELU", {"epi_act": GELU}),
          ("epi_act=7", {"epi_act": 7}), ("pad+1", {"pad": d["pad"] + 1}), ("stride=2", {"stride": 2}),
          ("T_out-1", {"T_out": d["T_out"] - 1}), ("alpha=0.5", {"alpha": 0.5}), ("pro_cscale=2", {"pro_cscale": 2.0}),
          ("Co+4", {"Co": d["Co"] + 4}), ("Co=24", {"Co": 24}), ("Ci-4", {"Ci": d["Ci"] - 4}), ("dil=64", {"dil": 64}),
          ("ks=5", {"ks": 5}), ("ks=13", {"ks": 13})]
    for dt in (F32, BF16, I32, F8, 9):
        if dt != d["in_dtype"]:
            m.append((f"in_dtype={dt}", {"in_dtype": dt}))
        if dt != d["out_dtype"]:
            m.append((f"out_dtype={dt}", {"out_dtype": dt}))
    for bit in range(3, 19):
        m.append((f"flags^{1 << bit}", {"flags": d["flags"] ^ (1 << bit)}))
    return m


def sweep_calls():
    """-> [(label, entry point, [conv dict, ...], rowln dict or None)]"""
    calls, bases = [], []

    def one(label, d, base=False):
        calls.append((label, "stzs_conv1d", [d], None))
        if base:
            bases.append((label, "stzs_conv1d", d, None))

    pairs = ((BF16, BF16), (BF16, F32), (F32, BF16), (F32, F32))
    # row counts on both sides of the launchers' grid thresholds against 256 CUs (B x T_out)
    BT_ = ((1, 100), (1, 4000), (2, 100), (5, 700), (8, 2100), (16, 4100), (64, 1024), (64, 1030), (64, 4100))
    # generic conv_mfma: dtype pairs x prologue activation x chunk width, flat and k3 / k7, split-K / DEEP / ticket / ring
    for (i, o), pa, cic in itertools.product(pairs, (NONE, LEAKY, SNAKE), (32, 64, 128)):
        one(f"mfma.k3 {i}{o} pa{pa} cic{cic}", conv(Ci=256, ks=3, cic=cic, ind=i, outd=o, pro_act=pa), base=(cic == 32 and pa != LEAKY))
        for sk, fl in ((2, 0), (256 // cic, 0), (256 // cic, SK_TICKET), (256 // cic, RING), (256 // cic, LINEAR_IDS)):
            if sk > 1:
                one(f"mfma.k3.sk{sk} {i}{o} pa{pa} cic{cic} f{fl}",
                    conv(B=1, Ci=256, ks=3, cic=cic, ind=i, outd=o, pro_act=pa, splitk=sk, flags=fl), base=(cic == 64 and pa == NONE and fl == 0))
                one(f"mfma.k3.sk{sk}.odd {i}{o} pa{pa} cic{cic} f{fl}",
                    conv(B=1, Ci=256, Co=100, ks=3, cic=cic, ind=i, outd=o, pro_act=pa, splitk=sk, flags=fl, ldy=100))
    for (i, o), cic in itertools.product(pairs, (32, 64, 128)):
        one(f"mfma.flat {i}{o} cic{cic}", conv(Ci=256, cic=cic, ind=i, outd=o), base=(cic == 32))
        for sk, fl, g in ((2, 0, 0), (256 // cic, 0, 0), (256 // cic, 0, 1), (256 // cic, SK_TICKET, 0)):
            if sk > 1:
                one(f"mfma.flat.sk{sk} {i}{o} cic{cic} f{fl} g{g}", conv(B=1, Ci=256, cic=cic, ind=i, outd=o, splitk=sk, flags=fl, gate=bool(g)))
    for ks, dil in ((1, 1), (3, 1), (7, 3), (11, 5), (7, 27), (11, 27), (3, 300), (11, 100)):  # up to and past the LDS capacity
        one(f"mfma.ks{ks}.dil{dil}", conv(Ci=256, ks=ks, dil=dil, cic=32))
        one(f"mfma.ks{ks}.dil{dil}.adain.stat", conv(Ci=256, ks=ks, dil=dil, cic=64, adain=True, stat=True, res=True, pro_act=LEAKY))
    one("mfma.ups", conv(Ci=256, Co=64, ups=4, cic=64, pro_act=LEAKY), base=True)
    one("mfma.ups.refl", conv(Ci=256, Co=64, ups=4, cic=64, refl=1))
    one("mfma.stride2", conv(Ci=256, ks=3, cic=32, stride=2, T_out=50), base=True)
    one("mfma.pro_part", conv(Ci=256, ks=3, cic=64, adain=True, pro_part=PTR["pro_part"], pro_nch=2, pro_T=100, pro_ld=256,
                              pro_mean=0, pro_rstd=0), base=True)
    for B, T in BT_:
        one(f"mfma.k3 B{B} T{T}", conv(B=B, T=T, Ci=256, ks=3, cic=64, res=True, acc=True, alpha=0.5))
    # A_DMA gemm_glds: every epilogue variant, both tile heights, split-K, fp8
    for o, r, a, ea in itertools.product((BF16, F32), (0, 1), (0, 1), (NONE, GELU, SILU, LEAKY)):
        for B, T in ((2, 100), (64, 1024)):  # (64 x 1024 rows: 512 128-row tiles, two rounds of 64-row ones)
            one(f"glds o{o} r{r} a{a} e{ea} B{B}", conv(B=B, T=T, Ci=256, flags=A_DMA, outd=o, res=bool(r), acc=bool(a), epi_act=ea),
                base=(B == 2 and r == a == 0 and ea == NONE))
            one(f"glds.f8 o{o} r{r} a{a} e{ea} B{B}", conv(B=B, T=T, Ci=256, cic=64, flags=A_DMA, ind=F8, outd=o, res=bool(r), acc=bool(a), epi_act=ea),
                base=(B == 2 and r == a == 0 and ea == NONE and o == BF16))
        for sk in (2, 4):
            one(f"glds.sk{sk} o{o} r{r} a{a} e{ea}", conv(B=1, Ci=512, flags=A_DMA, outd=o, res=bool(r), acc=bool(a), epi_act=ea, splitk=sk),
                base=(sk == 2 and r == a == 0 and ea == NONE and o == BF16))
    for o in (BF16, F32):  # the non-vector epilogue (EP -1), the gate, a scaled prologue (back to conv_mfma)
        one(f"glds.odd o{o}", conv(Ci=256, Co=100, flags=A_DMA, outd=o, ldy=100))
        for sk in (2, 4):
            one(f"glds.odd.sk{sk} o{o}", conv(B=1, Ci=512, Co=100, flags=A_DMA, outd=o, ldy=100, splitk=sk))
        one(f"glds.gate o{o}",conv(Ci=256, flags=A_DMA, outd=o, gate=True))
        one(f"glds.cscale o{o}", conv(Ci=256, flags=A_DMA, outd=o, pro_cscale=0.5))
        one(f"glds.f8.odd o{o}", conv(Ci=256, Co=100, cic=64, flags=A_DMA, ind=F8, outd=o, ldy=100))
    for B, T in BT_:
        one(f"glds B{B} T{T}", conv(B=B, T=T, Ci=256, flags=A_DMA))
    # X3 / F32 (precise generic forms)
    for (i, o), pa in itertools.product(pairs, (NONE, LEAKY, SNAKE)):
        one(f"x3.k3 {i}{o} pa{pa}", conv(Ci=64, ks=3, flags=X3, ind=i, outd=o, pro_act=pa), base=(pa == SNAKE and i == F32 and o == F32))
    for i, o in pairs:
        one(f"x3.flat {i}{o}", conv(Ci=64, flags=X3, ind=i, outd=o), base=(i == F32 and o == F32))
        one(f"x3.flat.stat {i}{o}", conv(Ci=64, flags=X3, ind=i, outd=o, stat=True))
        one(f"f32.k3 {i}{o}", conv(Ci=64, ks=3, flags=WF32, ind=i, outd=o), base=(i == F32 and o == F32))
        one(f"f32.k1 {i}{o}", conv(Ci=64, flags=WF32, ind=i, outd=o))
    for ks, dil in ((7, 3), (11, 5), (11, 27), (7, 60)):
        one(f"x3.ks{ks}.dil{dil}", conv(Ci=64, ks=ks, dil=dil, flags=X3, ind=F32, outd=F32))
        one(f"f32.ks{ks}.dil{dil}", conv(Ci=64, ks=ks, dil=dil, flags=WF32, ind=F32, outd=F32))
    # LANE16 (mrf_conv: the ring depth follows the grid) and NARROW32
    for pa, r, a in itertools.product((NONE, LEAKY, SNAKE), (0, 1), (0, 1)):
        for B, T in ((1, 100), (16, 4100)):
            one(f"lane16 pa{pa} r{r} a{a} B{B}", conv(B=B, T=T, Ci=256, ks=3, cic=128, flags=LANE16, pro_act=pa, res=bool(r), acc=bool(a)),
                base=(pa == SNAKE and r == 1 and a == 0 and B == 1))
    for ks, dil in ((7, 3), (11, 5), (11, 9), (11, 12), (3, 60)):
        one(f"lane16.ks{ks}.dil{dil}", conv(Ci=256, ks=ks, dil=dil, cic=128, flags=LANE16, pro_act=SNAKE))
        one(f"narrow32.ks{ks}.dil{dil}", conv(Ci=128, Co=22, ks=ks, dil=dil, cic=128, flags=NARROW32, outd=F32, pro_act=LEAKY, ldy=24))
    one("lane16.ups", conv(Ci=256, Co=64, ups=4, cic=128, flags=LANE16, pro_act=LEAKY), base=True)
    one("narrow32", conv(Ci=128, Co=22, ks=7, cic=128, flags=NARROW32, outd=F32, pro_act=LEAKY, ldy=24), base=True)
    one("narrow32.none", conv(Ci=128, Co=22, ks=7, cic=128, flags=NARROW32, outd=F32, ldy=24))
    # FRAG32 (mrfv): Snake forms, one / many chunks, R x A x alpha, the wide / 64-row / 128-row tiles and their flags
    for Ci, ks, r, a, al in itertools.product((128, 256), (3, 7, 11), (0, 1), (0, 1), (1.0, 0.5)):
        for (B, T), fl in itertools.product(((1, 100), (5, 700), (64, 1030)), (0, MRFV_NARROW, MRFV_T128, MRFV_NARROW | MRFV_T128)):
            one(f"frag32.snake Ci{Ci} ks{ks} r{r} a{a} al{al} B{B} f{fl}",
                conv(B=B, T=T, Ci=Ci, Co=256, ks=ks, cic=128, flags=FRAG32 | fl, pro_act=SNAKE, res=bool(r), acc=bool(a), alpha=al),
                base=(ks == 3 and r == 1 and a == 0 and al == 1.0 and B == 1 and fl == 0))
    for ks, pa, r in itertools.product((1, 3), (NONE, LEAKY), (0, 1)):
        for (B, T), fl in itertools.product(BT_, (0, MRFV_NARROW, MRFV_T128)):
            one(f"frag32.blk ks{ks} pa{pa} r{r} B{B} T{T} f{fl}",
                conv(B=B, T=T, Ci=512, Co=256, ks=ks, cic=128, flags=FRAG32 | fl, pro_act=pa, res=bool(r), adain=(ks == 3)),
                base=(B == 2 and fl == 0 and r == 1))
    for ks, dil in ((3, 8), (3, 9), (7, 5), (7, 6), (11, 6), (11, 7), (3, 40), (11, 4)):  # around sb_rows / sb_rows64
        one(f"frag32.ks{ks}.dil{dil}", conv(B=1, Ci=128, ks=ks, dil=dil, cic=128, flags=FRAG32, pro_act=SNAKE))
        one(f"frag32.ks{ks}.dil{dil}.B64", conv(B=64, T=1030, Ci=256, Co=256, ks=ks, dil=dil, cic=128, flags=FRAG32, pro_act=SNAKE))
    one("frag32.snake.stat", conv(Ci=128, ks=3, cic=128, flags=FRAG32, pro_act=SNAKE, stat=True), base=True)
    for Ci, r, nz, (B, T) in itertools.product((128, 256, 384, 512, 640), (0, 1), (0, 1), ((1, 40), (2, 100), (64, 130))):
        kw = dict(gate=True, res=True, ldr=32, bsr=32 * 1000) if nz else dict(res=bool(r))
        one(f"frag32.ups Ci{Ci} r{r} nz{nz} B{B}",
            conv(B=B, T=T, Ci=Ci, Co=128, ups=4, cic=128, flags=FRAG32 | (UPS_NOISE if nz else 0), pro_act=LEAKY, **kw),
            base=(Ci == 256 and B == 2 and not (nz and not r)))
    # FRAG32X3 (mrfx): conv, narrow, linear
    for Ci, ks, pa, r, a, al in itertools.product((128, 256), (3, 7, 11), (SNAKE, LEAKY, NONE), (0, 1), (0, 1), (1.0, 0.5)):
        for dil in (1, 5, 9):  # (5: k11 takes 64-row tiles)
            one(f"x3frag Ci{Ci} ks{ks} pa{pa} r{r} a{a} al{al} dil{dil}",
                conv(Ci=Ci, ks=ks, dil=dil, cic=128, flags=FRAG32X3, ind=F32, outd=F32, pro_act=pa, res=bool(r), acc=bool(a), alpha=al),
                base=(Ci == 256 and ks == 3 and pa == SNAKE and r == 1 and a == 0 and al == 1.0 and dil == 1))
    for dil in (1, 3, 9, 12, 20, 30):
        for ks in (3, 7, 11):
            one(f"x3frag.ks{ks}.dil{dil}", conv(Ci=128, ks=ks, dil=dil, cic=128, flags=FRAG32X3, ind=F32, outd=F32, pro_act=SNAKE))
        one(f"x3frag.narrow dil{dil}", conv(Ci=128, Co=22, ks=7, dil=dil, cic=128, flags=FRAG32X3, ind=F32, outd=F32, pro_act=LEAKY, ldy=24),
            base=(dil == 1))
    for g, r, a, ea in itertools.product((0, 1), (0, 1), (0, 1), (NONE, GELU, SILU, LEAKY)):
        one(f"x3frag.lin g{g} r{r} a{a} e{ea}",
            conv(Ci=256, cic=128, flags=FRAG32X3, ind=F32, outd=F32, gate=bool(g), res=bool(r), acc=bool(a), epi_act=ea),
            base=(g == r == a == 0 and ea == NONE))
    one("x3frag.adain.stat", conv(Ci=256, ks=3, cic=128, flags=FRAG32X3, ind=F32, outd=F32, pro_act=LEAKY, adain=True, stat=True, alpha=0.5))
    # ROWS (gemm_rows) and stzs_ln_linear without / with a LayerNorm
    rp = ((BF16, BF16), (BF16, F32), (F32, F32), (F32, BF16))
    for (i, o), Ci, sk, ea, (B, T) in itertools.product(rp, (128, 256, 512, 1024, 2048, 4096), (0, 2, 4, 16),
                                                        (NONE, GELU, SILU, LEAKY), ((1, 20), (1, 64), (1, 65), (2, 100))):
        d = conv(B=B, T=T, Ci=Ci, Co=200, flags=ROWS, ind=i, outd=o, splitk=sk, epi_act=ea, res=(ea == NONE))
        isb = (i, o) == (BF16, BF16) and Ci == 512 and ea == NONE and B == 2 and sk in (0, 2)
        one(f"rows {i}{o} Ci{Ci} sk{sk} e{ea} B{B} T{T}", d, base=isb)
        if T != 64:
            calls.append((f"plain {i}{o} Ci{Ci} sk{sk} e{ea} B{B} T{T}", "stzs_ln_linear", [dict(d, flags=0)], None))
            if isb:
                bases.append((calls[-1][0], "stzs_ln_linear", dict(d, flags=0), None))
    for (li, o), Cn, ea, R in itertools.product(((F32, BF16), (F32, F32), (BF16, BF16), (BF16, F32)), (128, 256, 512, 1024),
                                                (NONE, GELU, SILU, LEAKY), (20, 200)):
        d = conv(B=1, T=R, Ci=Cn, Co=200, ind=BF16, outd=o, epi_act=ea, x=0)
        calls.append((f"lnlin {li}{o} C{Cn} e{ea} R{R}", "stzs_ln_linear", [d], rowln(R, Cn, li)))
        if Cn == 256 and ea == NONE and R == 20:
            bases.append((calls[-1][0], "stzs_ln_linear", d, rowln(R, Cn, li)))
    ln_bad = (("x=NULL", dict(x=0)), ("lens", dict(lens=PTR["gate"])), ("C+32", dict(C=288)), ("R+1", dict(R=21)), ("ldx+4", dict(ldx=260)),
              ("gdiv=0", dict(gdiv=0)), ("x+8", dict(x=PTR["x"] + 8)), ("gs+4", dict(gs=260)), ("G+16", dict(G=PTR["pro_gb"] + 16)),
              ("bs+4", dict(bs=260)), ("Bt+16", dict(Bt=PTR["pro_mean"] + 16)), ("out=f32", dict(out_dtype=F32)), ("act=GELU", dict(act=GELU)),
              ("in=i32", dict(in_dtype=I32)), ("G=NULL", dict(G=0)), ("Bt=NULL", dict(Bt=0)))
    for lab, ch in ln_bad:
        calls.append((f"lnlin.ln {lab}", "stzs_ln_linear", [conv(B=1, T=20, Ci=256, Co=200, x=0)], rowln(20, 256, F32, **ch)))
    # ragged frame lengths (stzs_conv_args.t_lens): the generic conv_mfma path and the register-direct k3 block form
    # launch their own instances ("tlens ..."); every other form or combination is refused before any runtime call
    # ("tlens.bad ...": STZS_EINVAL, nothing launched)
    TL = PTR["t_lens"]
    for (i, pa, mul) in itertools.product((BF16, F32), (NONE, LEAKY), (0, 2)):
        one(f"tlens mfma.k3 {i}{i} pa{pa} mul{mul}", conv(B=4, T=200, Ci=64, Co=32, ks=3, cic=64, ind=i, outd=i, pro_act=pa, adain=True,
                                                       stat=True, res=True, alpha=0.5, t_lens=TL, t_lens_mul=mul))
    one("tlens mfma.k3 linear_ids", conv(B=4, T=200, Ci=64, Co=32, ks=3, cic=64, flags=LINEAR_IDS, t_lens=TL))
    for pa, r, ((B, T), fl) in itertools.product((NONE, LEAKY), (0, 1), (((2, 100), 0), ((2, 100), MRFV_T128), ((64, 1030), 0),
                                                                    ((64, 1030), MRFV_NARROW))):
        one(f"tlens frag32.blk pa{pa} r{r} B{B} T{T} f{fl}",
            conv(B=B, T=T, Ci=512, Co=256, ks=3, cic=128, flags=FRAG32 | fl, pro_act=pa, res=bool(r), adain=True, stat=True,
                 res_tdiv=1 + r, t_lens=TL, t_lens_mul=2 * r))
    g3 = conv(B=4, T=200, Ci=64, Co=32, ks=3, cic=64, adain=True, pro_act=LEAKY, t_lens=TL)
    f3 = conv(B=4, T=200, Ci=256, Co=256, ks=3, cic=128, flags=FRAG32, adain=True, pro_act=LEAKY, t_lens=TL)
    for lab, d in (("mfma snake", dict(g3, pro_act=SNAKE, pro_alpha=PTR["pro_alpha"])), ("mfma bf16->f32", dict(g3, out_dtype=F32)),
                   ("mfma f32->bf16", dict(g3, in_dtype=F32)),
                   ("mfma splitk", dict(g3, B=1, Ci=256, ci_pad=256, ldx=256, splitk=4, splitk_ws=PTR["splitk_ws"], splitk_ctr=PTR["splitk_ctr"])),
                   ("mfma pro_part", dict(g3, pro_part=PTR["pro_part"], pro_nch=2, pro_T=200, pro_ld=64)),
                   ("mfma stride 2", dict(g3, stride=2, T_out=100)), ("mfma T_out-1", dict(g3, T_out=199)),
                   ("mfma ups", conv(Ci=256, Co=64, ups=4, cic=64, pro_act=LEAKY, t_lens=TL)),
                   ("mfma flat", conv(Ci=256, cic=64, t_lens=TL)), ("glds", conv(Ci=256, flags=A_DMA, t_lens=TL)),
                   ("mfma scalar epilogue", dict(g3, Co=30, ldy=30)), ("mfma mul 3", dict(g3, t_lens_mul=3)),
                   ("mfma mul -1", dict(g3, t_lens_mul=-1)), ("mfma t_lens+2", dict(g3, t_lens=TL + 2)),
                   ("frag32 snake", dict(f3, pro_act=SNAKE, pro_alpha=PTR["pro_alpha"])), ("frag32 ks 7", dict(f3, ks=7, pad=3)),
                   ("frag32 ks 1 shortcut", conv(B=4, T=200, Ci=256, Co=256, cic=128, flags=FRAG32, t_lens=TL)),
                   ("frag32 acc_in", dict(f3, acc_in=PTR["acc_in"], lda=256, bsa=200 * 256)),
                   ("frag32 ups", conv(Ci=256, Co=128, ups=4, cic=128, flags=FRAG32, pro_act=LEAKY, t_lens=TL)),
                   ("lane16", conv(Ci=256, ks=3, cic=128, flags=LANE16, pro_act=LEAKY, t_lens=TL)),
                   ("narrow32", conv(Ci=128, Co=22, ks=7, cic=128, flags=NARROW32, outd=F32, pro_act=LEAKY, ldy=24, t_lens=TL)),
                   # (the precise forms take fp32 rows with lengths, --ragged-precise-cases: what they still refuse)
                   ("x3 bf16", conv(Ci=64, ks=3, flags=X3, ind=BF16, outd=BF16, t_lens=TL)),
                   ("f32", conv(Ci=64, ks=3, flags=WF32, ind=F32, outd=F32, t_lens=TL)),
                   ("x3frag ks 7", conv(Ci=256, ks=7, cic=128, flags=FRAG32X3, ind=F32, outd=F32, pro_act=LEAKY, t_lens=TL)),
                   ("rows", conv(B=1, T=20, Ci=512, Co=200, flags=ROWS, t_lens=TL))):
        one(f"tlens.bad {lab}", d)

    # groups: the MRF trio, the DEEP split-K pair, their fallbacks (one after the other)
    def trio(Ci=128, B=1, T=100, r=True, flags=FRAG32, **kw):
        return [conv(B=B, T=T, Ci=Ci, Co=128, ks=k, cic=128, flags=flags, pro_act=SNAKE, res=r, **kw) for k in (3, 7, 11)]

    groups = [("trio.n1", trio()), ("trio.n1.nores", trio(r=False)), ("trio.multi", trio(Ci=256)), ("trio.multi.nores", trio(Ci=256, r=False)),
              ("trio.big", trio(B=64, T=1030)), ("trio.alpha", trio(alpha=0.5)), ("trio.acc", trio(acc=True)),
              ("trio.order", trio()[::-1]), ("trio.t128", trio(flags=FRAG32 | MRFV_T128)), ("trio.x3", trio(flags=FRAG32X3, ind=F32, outd=F32)),
              ("trio.two", trio()[:2]), ("trio.one", trio()[:1])]
    for pa in (NONE, LEAKY, SNAKE):
        groups.append((f"pair pa{pa}", [conv(B=1, Ci=256, ks=3, cic=64, splitk=4, adain=True, pro_act=pa) for _ in range(2)]))
    groups += [("pair.mixed act", [conv(B=1, Ci=256, ks=3, cic=64, splitk=4, pro_act=pa) for pa in (LEAKY, NONE)]),
               ("pair.f32", [conv(B=1, Ci=256, ks=3, cic=64, splitk=4, outd=F32) for _ in range(2)]),
               ("pair.nosplit", [conv(B=1, Ci=256, ks=3, cic=64) for _ in range(2)]),
               ("pair.ticket", [conv(B=1, Ci=256, ks=3, cic=64, splitk=4, flags=SK_TICKET) for _ in range(2)]),
               ("pair.flat", [conv(B=1, Ci=256, cic=64, splitk=4) for _ in range(2)]),
               ("pair.frag32", trio()[:2]),
               ("tlens.bad trio", trio(t_lens=PTR["t_lens"])),
               ("tlens.bad pair", [conv(B=1, Ci=256, ks=3, cic=64, splitk=4, adain=True, t_lens=PTR["t_lens"]) for _ in range(2)]),
               ("tlens pair.nosplit", [conv(B=1, Ci=256, ks=3, cic=64, t_lens=PTR["t_lens"]) for _ in range(2)]),
               ("pair.pro_part one", [conv(B=1, Ci=256, ks=3, cic=64, splitk=4, adain=True, **kw) for kw in
                                      ({}, dict(pro_part=PTR["pro_part"], pro_nch=2, pro_T=100, pro_ld=256))]),
               ("pair.pro_part both", [conv(B=1, Ci=256, ks=3, cic=64, splitk=4, adain=True, pro_part=PTR["pro_part"], pro_nch=2,
                                            pro_T=100, pro_ld=256) for _ in range(2)])]
    # the ragged decoder (t_lens_rows = 1: an utterance's own row count): the register-direct Snake convs, the
    # polyphase ConvTranspose and the narrow conv_post form launch instances of their own ("trows ..."); every other form
    # or combination is refused before any runtime call ("trows.bad ...": STZS_EINVAL, nothing launched)
    TR = dict(t_lens=TL, t_lens_rows=1)
    epi = (("plain", {}), ("res.stat", dict(res=True, stat=True)), ("res.alpha", dict(res=True, alpha=1 / 3)),
           ("res.acc.alpha", dict(res=True, acc=True, alpha=1 / 3)), ("res.acc", dict(res=True, acc=True)))
    for Ci, ks, (elab, ekw), (B, T) in itertools.product((128, 256), (3, 7, 11), epi, ((4, 200), (64, 1030))):
        for fl in ((0, MRFV_NARROW) if (Ci == 256 and B == 64) else (0,)):
            one(f"trows frag32.snake Ci{Ci} ks{ks} {elab} B{B} f{fl}",
                conv(B=B, T=T, Ci=Ci, Co=256, ks=ks, dil=5 if ks == 11 else 1, cic=128, flags=FRAG32 | fl, pro_act=SNAKE,
                     adain=True, **ekw, **TR))
    for Ci, r, nz, refl, (B, T) in itertools.product((128, 256, 384, 512), (0, 1), (0, 1), (0, 1), ((4, 40), (64, 130))):
        kw = dict(gate=True, res=True, ldr=32, bsr=32 * 1000) if nz else dict(res=bool(r))
        one(f"trows frag32.ups Ci{Ci} r{r} nz{nz} refl{refl} B{B}",
            conv(B=B, T=T, Ci=Ci, Co=128, ups=4, cic=128, flags=FRAG32 | (UPS_NOISE if nz else 0), pro_act=LEAKY, refl=refl,
                 **kw, **TR))
    n7 = conv(B=4, T=200, Ci=128, Co=22, ks=7, cic=128, flags=NARROW32, outd=F32, pro_act=LEAKY, ldy=24, **TR)
    one("trows narrow32", n7)
    one("trows narrow32 mul1", dict(n7, t_lens_mul=1))
    s3 = conv(B=4, T=200, Ci=256, Co=256, ks=3, cic=128, flags=FRAG32, pro_act=SNAKE, adain=True, **TR)
    for lab, d in (("mfma snake", conv(B=4, T=200, Ci=64, Co=32, ks=3, cic=64, adain=True, pro_act=SNAKE, **TR)),
                   ("mfma leaky", conv(B=4, T=200, Ci=64, Co=32, ks=3, cic=64, adain=True, pro_act=LEAKY, **TR)),
                   ("lane16", conv(Ci=256, ks=3, cic=128, flags=LANE16, pro_act=SNAKE, **TR)),
                   # (the precise forms take fp32 rows with row counts, --ragged-precise-cases: never bf16 rows)
                   ("x3frag bf16", conv(Ci=256, ks=3, cic=128, flags=FRAG32X3, ind=BF16, outd=BF16, pro_act=SNAKE, **TR)),
                   ("x3 bf16", conv(Ci=64, ks=3, flags=X3, ind=BF16, outd=BF16, **TR)),
                   ("rows", conv(B=1, T=20, Ci=512, Co=200, flags=ROWS, **TR)),
                   ("glds", conv(Ci=256, flags=A_DMA, **TR)),
                   ("splitk", dict(s3, B=1, splitk=2, splitk_ws=PTR["splitk_ws"], splitk_ctr=PTR["splitk_ctr"])),
                   ("mul 2", dict(s3, t_lens_mul=2)), ("mul -1", dict(s3, t_lens_mul=-1)), ("rows 2", dict(s3, t_lens_rows=2)),
                   ("rows -1", dict(s3, t_lens_rows=-1)), ("rows 1 no lengths", dict(s3, t_lens=0)), ("lengths+2", dict(s3, t_lens=TL + 2)),
                   ("stride 2", dict(s3, stride=2, T_out=100)), ("T_out-1", dict(s3, T_out=199)),
                   ("pro_part", dict(s3, pro_part=PTR["pro_part"], pro_nch=2, pro_T=200, pro_ld=256)),
                   ("frag32 blk leaky", dict(s3, pro_act=LEAKY)), ("frag32 blk none", dict(s3, pro_act=NONE)),
                   ("frag32 ks 1 shortcut", conv(B=4, T=200, Ci=256, Co=256, cic=128, flags=FRAG32, **TR)),
                   ("frag32 acc no res", dict(s3, acc_in=PTR["acc_in"], lda=256, bsa=200 * 256)),
                   ("frag32 alpha no res", dict(s3, alpha=0.5)),
                   ("frag32 ups mul 2", conv(Ci=256, Co=128, ups=4, cic=128, flags=FRAG32, pro_act=LEAKY, t_lens=TL, t_lens_rows=1, t_lens_mul=2)),
                   ("frag32 ups rows 2", conv(Ci=256, Co=128, ups=4, cic=128, flags=FRAG32, pro_act=LEAKY, t_lens=TL, t_lens_rows=2)),
                   ("mfma ups", conv(Ci=256, Co=64, ups=4, cic=64, pro_act=LEAKY, **TR)),
                   ("narrow32 rows 2", dict(n7, t_lens_rows=2)), ("narrow32 mul 2", dict(n7, t_lens_mul=2))):
        one(f"trows.bad {lab}", d)
    # (groups with lengths run one stzs_conv1d at a time: the trio and pair launches stay length-free)
    groups += [("trows trio", trio(Ci=256, adain=True, **TR)), ("trows.bad trio", trio(adain=True, t_lens=TL, t_lens_rows=2)),
               ("trows.bad trio mul 2", trio(adain=True, t_lens_mul=2, **TR))]
    for lab, ds in groups:
        calls.append((f"group {lab}", "stzs_conv1d_group", ds, None))
    for lab, ds in (groups[0], groups[2], groups[12]):  # a defect in one member of a group
        for k in range(len(ds)):
            for mlab, ch in mutants(ds[k]):
                calls.append((f"group {lab} [{k}] {mlab}", "stzs_conv1d_group", ds[:k] + [dict(ds[k], **ch)] + ds[k + 1:], None))
    calls.append(("group n=0", "stzs_conv1d_group", [], None))
    # single-defect mutants of every base; a few multi-defect calls
    for lab, fn, d, ln in bases:
        for mlab, ch in mutants(d):
            calls.append((f"{lab} | {mlab}", fn, [dict(d, **ch)], ln))
    multi = [("multi all-zero", {}), ("multi zero+frag32", dict(flags=FRAG32)), ("multi zero+x3frag", dict(flags=FRAG32X3)),
             ("multi zero+rows", dict(flags=ROWS)), ("multi null x + B 0", conv(Ci=256, ks=3, x=0, B=0)),
             ("multi frag32: f8 + splitk + lane16", conv(Ci=128, ks=3, cic=128, flags=FRAG32 | LANE16, ind=F8, splitk=2)),
             ("multi rows: ks 3 + co_pad + x+4", conv(Ci=512, ks=3, flags=ROWS, co_pad=192, x=PTR["x"] + 4)),
             ("multi x3frag: rows + ldx + w+4", conv(Ci=256, ks=3, cic=128, flags=FRAG32X3 | ROWS, ldx=12, w=PTR["w"] + 4)),
             ("multi mfma: cic 48 + T_out 0 + gelu", conv(Ci=256, ks=3, cic=48, T_out=0, pro_act=GELU))]
    for lab, d in multi:
        calls.append((lab, "stzs_conv1d", [d], None))
        calls.append((lab + " (ln_linear)", "stzs_ln_linear", [d], None))
    return calls


def sweep(lib, out):
    L = _load(lib, out)
    from stzs import _lib
    rcs = []
    for label, fn, ds, ln in sweep_calls():
        arr = (_lib.ConvArgs * max(len(ds), 1))()
        for k, d in enumerate(ds):
            for f, v in d.items():
                setattr(arr[k], f, v)
        L.hip_record_mark(f"call {fn} {label}".encode())
        if fn == "stzs_conv1d":
            rc = L.stzs_conv1d(C.byref(arr[0]), None)
        elif fn == "stzs_conv1d_group":
            rc = L.stzs_conv1d_group(arr, len(ds), None)
        else:
            r = None
            if ln is not None:
                r = _lib.RowLNArgs()
                for f, v in ln.items():
                    setattr(r, f, v)
            rc = L.stzs_ln_linear(C.byref(arr[0]), C.byref(r) if r is not None else None, None)
        L.hip_record_mark(f"rc {rc}".encode())
        rcs.append(rc)
    ok = sum(rc >= 0 for rc in rcs)
    print(f"sweep: {len(rcs)} calls, {ok} accepted, {len(rcs) - ok} rejected -> {out}")


# ---- mode (c): the linears' probe table -----------------------------------------------------------------------------
def linear_cases(lib, out):
    """every case of tests/refops.py linear_cases() (the table tests/test_gpu_linear_probe.py runs on the device) through
    the engine's routing and the native dispatch, with the operands the GPU test builds (on the host): one "call
    <case id>" marker per case, then the launch it made"""
    L = _load(lib, out)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refops as R
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.spec import SPEC_TINY
    eng = StyleTTSZS(SPEC_TINY, init_params(SPEC_TINY, 0), device="cpu")
    eng.stream = lambda: C.c_void_p(0)  # (no device: the null stream, as tools/launch_trace.py)
    cases = R.linear_cases(256)  # (the stand-in reports 256 CUs)
    for c in cases:
        x, sx, _ = R.lin_make_x(c)
        _, xa = R.lin_x_layout(c, x, True)
        _, ya = R.lin_y_layout(c, True)
        cw = R.lin_onehot(c, 0)
        L.hip_record_mark(f"call {R.lin_id(c)}".encode())
        R.lin_launch(eng, c, cw, xa, ya, x_scale=sx)
        L.hip_record_mark(b"rc 0")
    print(f"linear cases: {len(cases)} -> {out}")


# ---- mode (d): the precise convs' probe, exact-sum and dense tables ------------------------------------------------
def precise_cases(lib, out):
    """every case of tests/refops.py precise_probe_cases() / precise_exact_cases() / precise_dense_cases() (the tables
    tests/test_gpu_precise_probe.py runs on the device) through the engine's routing and the native dispatch, with the
    operands the GPU test builds (on the host): one "call <table> <case id>" marker per case, then the launch it made"""
    import ctypes
    L = _load(lib, out)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refops as R
    from stzs.engine import StyleTTSZS
    from stzs.params import init_params
    from stzs.spec import SPEC_TINY
    eng = StyleTTSZS(SPEC_TINY, init_params(SPEC_TINY, 0), device="cpu")
    eng.stream = lambda: C.c_void_p(0)  # (no device: the null stream, as tools/launch_trace.py)

    def call(label, a):
        L.hip_record_mark(f"call {label}".encode())
        rc = eng.lib.stzs_conv1d(ctypes.byref(a), eng.stream())
        L.hip_record_mark(f"rc {rc}".encode())

    n = 0
    for c in R.precise_probe_cases():
        o = R.px_make_ops(c)
        for poisoned in (True, False):
            w = R.delta_weights_T(c.Ci, c.Co, c.k, 0, 0) if c.ups else R.delta_weights(c.Co, c.Ci, c.k, 0, 0)
            cw = R.px_pack(c, w, None, (c.kern, c.Co, c.Ci, c.k, c.ups))
            a = R.px_args(eng, c, cw, R.px_layout(c, o, poisoned), R.px_y(c, poisoned)[1])
            call(f"probe{'' if poisoned else '.compact'} {R.px_id(c)}", a)
            n += 1
    for c, seed, e in R.precise_exact_cases():
        ops, _ = R.px_exact_operands(c, seed, e)
        w = ops["w"].transpose(0, 1).contiguous() if c.ups else ops["w"]
        a, keep = R.px_dense_args(eng, c, w, ops["b"], dict(x=ops["x"], mean=None, alpha=None), res=ops["res"],
                                  res_tdiv=e["res_tdiv"], acc=ops["acc"], alpha=e["alpha"], beta=e["beta"], gate=ops["gate"],
                                  stat=e["stat"])
        call(f"exact {R.px_exact_id((c, seed, e))}", a)
        n += 1
    for c, e in R.precise_dense_cases():
        d = R.px_dense_operands(c, e)
        a, keep = R.px_dense_args(eng, c, d["w"], d["b"], R.px_make_ops(c), res=d["res"], res_tdiv=e["res_tdiv"], acc=d["acc"],
                                  alpha=e["alpha"], beta=e["beta"], gate=d["gate"], stat=e["stat"])
        call(f"dense {R.px_dense_id((c, e))}", a)
        n += 1
    print(f"precise cases: {n} -> {out}")


# ---- mode (e): the precise convs with per-row lengths ---------------------------------------------------------------
def ragged_precise_args(c, lengths=True):
    """a case of tests/ragged_precise_cases.py -> the stzs_conv_args fields (fixed fake pointers); lengths=False: the
    same problem without t_lens (its non-ragged sibling)"""
    fx3 = c["form"] == "fx3"
    act = {"snake": SNAKE, "leaky": LEAKY, "none": NONE}[c["act"]]
    d = conv(B=c["B"], T=c["T"], Ci=c["Ci"], Co=c["Co"], ks=c["ks"], dil=c["dil"], cic=128 if fx3 else 32,
             flags=FRAG32X3 if fx3 else X3, ind=F32, outd=F32, res=c["res"], acc=c["acc"], pro_act=act, adain=c["adain"],
             stat=c["stat"], alpha=c["alpha"], ups=c["ups"], res_tdiv=c["tdiv"], refl=c["refl"])
    d["ci_pad"] = rup(c["Ci"], 128 if c["Ci"] > 64 else 64 if c["Ci"] > 32 else 32)  # (stzs/weights.py pack_conv)
    d["ldx"], d["bsx"] = d["ci_pad"], c["T"] * d["ci_pad"]
    if c["Co"] == 22:  # (conv_post: 24-column rows)
        d["ldy"], d["bsy"] = 24, c["T"] * 24
    if c["ups"]:
        d["ups_pad"] = c["ups"] // 2
    if lengths:
        d.update(t_lens=PTR["t_lens"], t_lens_rows=c["mode"], t_lens_mul=c["mul"])
    d.update(c["over"])
    return d


def ragged_precise_cases(lib, out):
    """every launch shape of tests/test_gpu_ragged_precise_kernels.py (tests/ragged_precise_cases.py) through the native
    dispatch: "call rag <label>" with the lengths, "call uni <label>" the same problem without them (the non-ragged
    sibling: same grid, same LDS bytes, the kernel without RAG), "call bad <label>" the refusals"""
    L = _load(lib, out)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ragged_precise_cases as RP
    from stzs import _lib

    def call(label, d):
        a = _lib.ConvArgs()
        for f, v in d.items():
            setattr(a, f, v)
        L.hip_record_mark(f"call {label}".encode())
        rc = L.stzs_conv1d(C.byref(a), None)
        L.hip_record_mark(f"rc {rc}".encode())

    acc, bad = RP.accepted(), RP.refused()
    for c in acc:
        call("rag " + c["label"], ragged_precise_args(c))
        call("uni " + c["label"], ragged_precise_args(c, lengths=False))
    for c in bad:
        call("bad " + c["label"], ragged_precise_args(c))
    print(f"ragged precise cases: {len(acc)} accepted (each with its non-ragged sibling), {len(bad)} refused -> {out}")


# ---- coverage -----------------------------------------------------------------------------------------------------
def registered(objdir, names=CONV_OBJECTS):
    """{object: set of registered kernel names}, from the objects' host stubs (nm)"""
    out = {}
    for n in names:
        syms = subprocess.run(["nm", os.path.join(objdir, n + ".o")], capture_output=True, text=True, check=True).stdout
        ks = set()
        for s in re.findall(r"\S*__device_stub__\S*", syms):
            # _Z<N>__device_stub__name... -> _Z<N-15>name... (the stub's mangled name without its 15-character prefix)
            # (the anonymous namespace's "12_GLOBAL__N_1" ends in a digit: set aside while the length is rewritten)
            s = re.sub(r"(\d+)__device_stub__", lambda m: str(int(m.group(1)) - 15), s.replace("_GLOBAL__N_1", "@"))
            ks.add(s.replace("@", "_GLOBAL__N_1"))
        out[n] = ks
    return out


def coverage(objdir, traces):
    seen = set()
    for t in traces:
        seen.update(ln.split()[1] for ln in open(t).read().splitlines() if ln.startswith("L "))
    total = missing = 0
    for n, ks in registered(objdir).items():
        miss = sorted(ks - seen)
        total, missing = total + len(ks), missing + len(miss)
        print(f"{n}: {len(ks)} registered, {len(miss)} never launched")
        for k in miss:
            d = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip() or k
            print(f"    {d}")
    print(f"conv family: {total} registered, {total - missing} launched, {missing} never launched")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--objects", default=OBJECTS, help="directory of the library build's objects")
    ap.add_argument("--lib", help="where to link the trace library (default OBJECTS/libstzs_trace.so)")
    ap.add_argument("--out", default="dispatch_trace.txt", help="the trace file")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--synth", choices=("tiny", "v0"))
    g.add_argument("--sweep", action="store_true")
    g.add_argument("--coverage", nargs="+", metavar="TRACE")
    g.add_argument("--linear-cases", action="store_true")
    g.add_argument("--precise-cases", action="store_true")
    g.add_argument("--ragged-precise-cases", action="store_true")
    a = ap.parse_args()
    if a.coverage:
        return coverage(a.objects, a.coverage)
    lib = build_trace_lib(a.objects, a.lib)
    out = os.path.abspath(a.out)
    if a.synth:
        synth(a.synth, lib, out)
    elif a.linear_cases:
        linear_cases(lib, out)
    elif a.precise_cases:
        precise_cases(lib, out)
    elif a.ragged_precise_cases:
        ragged_precise_cases(lib, out)
    else:
        sweep(lib, out)


if __name__ == "__main__":
    main()
