"""Every GEMM kernel instance behind csrc/gemm_plan.h: the case table, the instance each case claims read off the library's own
plan text, and the operands (used by test_gpu_gemm_instances.py and its CPU guard test_gemm_cases.py).  The pattern is
tail_cases.py's.

An instance is a set of template arguments the launchers can ask for.  Its key is
    (family, MA, OUT, VS, MF, AL, NG, WN, WM, IM, NTT, KS, NONNEG)
read from capi.gemm_plan_text under the case's knobs; KS (cin / 32) is a template argument of the wide kernel only and 0
elsewhere; NONNEG (relu / relu6: the packed requantisation) splits the wide kernel's int8 instances and is 0 elsewhere -- no plan
prints it, launch_wide_t derives it from the activation.  expected_keys() enumerates the set from first principles (what
run_gemm_t, run_tr_tile and launch_wide_t can instantiate); the guard holds its per-family counts to
tools/dump_gemm_plans.INSTANCES and the table to exactly that set minus UNREACHABLE.

A case is (shape, knobs, output kinds, classes) plus the instance it claims without OUT: one launch per output kind and
activation.  shape is tail_cases' (n, cin, h, w, cout, k, pads, stride, dilation, groups).  The pointer offsets are
POINTER_CASES': (x bytes, y elements) off the vector alignment on one or two cases per family; the plan of such a launch is the
text with TAIL_UNALIGNED (y) / TAIL_X_UNALIGNED (x), and it claims an instance of its own.
`classes` are predicates on the plan (CLASSES): the smallest shapes at which a K loop, a column walk or a row walk changes path.

The test families: private, lds, ring (NG = 0), areg (NG > 0), tr_im (implicit GEMM on gemm_tr_*), tr_plain (GEMM_TR = 2) and
wide.  Operands are edge_cases' (dyadic folded scales, quarter biases, one output of every channel on an anchor); the
reference is always plref.conv2d_acc + plref.epilogue.  No device code here."""
import functools

import numpy as np

import dwconv_cases as D
import edge_cases as E
import tail_cases as T

P0, P1, P2 = T.P0, T.P1, T.P2
GEMM, IMPLICIT = T.GEMM, T.IMPLICIT
TAIL_UNALIGNED, TAIL_X_UNALIGNED = 8, 16  # capi.TAIL_*
OUTS = ("i32", "f32", "i8")
FAMILIES = ("private", "lds", "ring", "areg", "tr_im", "tr_plain", "wide")
KEY_FIELDS = ("family", "MA", "OUT", "VS", "MF", "AL", "NG", "WN", "WM", "IM", "NTT", "KS", "NONNEG")
TR_TILES = ((4, 1), (2, 2), (4, 2), (1, 4), (2, 4))  # (WN, WM): gemm_tr_4x1, 2x2, 4x2, 1x4, 2x4
WIDE_PAIRS = tuple((4, ks) for ks in (4, 8, 16, 32)) + tuple((ntt, ks) for ntt in (7, 8) for ks in (4, 8, 16))
DWORD_FORMS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1))  # (AL, VS, MF): the four forms run_gemm_t launches


def make_key(family, out, **f):
    f = dict(f, family=family, OUT=E.OUT_KINDS[out] if isinstance(out, str) else out)
    assert set(f) <= set(KEY_FIELDS), f
    return tuple(f.get(k, 0) for k in KEY_FIELDS)


def expected_keys():
    """Every instance the library builds, from the launchers' own dispatch (gemm_i8.hip run_gemm_t, gemm_tr_i8.hip run_tr_tile,
    gemm_wide_kernel.h launch_wide_t)."""
    keys = set()
    for out in OUTS:
        for ma in (1, 2):
            for fam in ("private", "lds"):
                keys |= {make_key(fam, out, MA=ma, AL=al, VS=vs, MF=mf) for al, vs, mf in DWORD_FORMS}
            keys |= {make_key("ring", out, MA=ma, VS=vs, MF=mf) for vs in (0, 1) for mf in (0, 1)}
        keys |= {make_key("ring", out, MA=2, MF=1, VS=vs, NG=ng) for ng in (1, 2, 4, 8) for vs in (0, 1)}
        keys |= {make_key("tr", out, WN=wn, WM=wm, IM=im) for wn, wm in TR_TILES for im in (0, 1)}
        for ntt, ks in WIDE_PAIRS:
            keys |= {make_key("wide", out, NTT=ntt, KS=ks, NONNEG=nn) for nn in ((0, 1) if out == "i8" else (0,))}
    return keys


def plan_family(key):
    """The family tools/dump_gemm_plans.INSTANCES counts a key under."""
    return key[0]


def test_family(key):
    """The test family (FAMILIES) a key runs in."""
    f = dict(zip(KEY_FIELDS, key))
    if f["family"] == "ring":
        return "areg" if f["NG"] else "ring"
    if f["family"] == "tr":
        return "tr_im" if f["IM"] else "tr_plain"
    return f["family"]


# instances no descriptor and no knob setting reaches through the C ABI: {key: the line that excludes it}.  (None: every
# instance the library builds can be launched through plhip_conv2d_int8 under some knob setting.)
UNREACHABLE = {}


def _c(name, fam, shape, knobs, claim, classes=(), outs=OUTS, seeds=None):
    """claim: the key's fields without family, OUT and NONNEG.  seeds: one per activation of E.ACTS, searched (find_seeds)."""
    impl = IMPLICIT if fam == "tr_im" else GEMM
    return {"name": name, "family": fam, "shape": shape, "knobs": dict(knobs), "claim": dict(claim), "classes": tuple(classes),
            "outs": tuple(outs), "seeds": seeds, "impl": impl}


def _g(n, cin, h, w, cout):
    return (n, cin, h, w, cout, 1, P0, 1, 1, 1)


def _dword_cases(fam, variant):
    kn = {"GEMM_VARIANT": variant}
    p = fam[0]
    return [
        _c(p + "1_ks1_7x7", fam, _g(2, 32, 7, 7, 24), kn, dict(MA=1), ("ks1", "hw_odd", "m_tail", "spans_images", "ragged_n")),
        _c(p + "1_ks2_m32", fam, _g(3, 64, 4, 4, 32), kn, dict(MA=1, AL=1, VS=1, MF=1), ("ks2", "hw_quad", "m_full"), seeds=(0,) * 7),
        _c(p + "1_ks3_m24", fam, _g(2, 96, 4, 5, 24), kn, dict(MA=1, AL=1, VS=1), ("ks3", "m_tail")),
        _c(p + "1_m136", fam, _g(2, 96, 4, 4, 136), kn, dict(MA=1, AL=1, VS=1), ("m_idle", "m_tail")),
        _c(p + "2_k72_m64", fam, _g(2, 72, 4, 4, 64), kn, dict(MA=2, AL=1, VS=1, MF=1), ("k_ragged", "m_full")),
        _c(p + "2_k100_m48", fam, _g(2, 100, 6, 6, 48), kn, dict(MA=2, AL=1, VS=1), ("k_ragged", "m_tail")),
        _c(p + "2_7x7_m64", fam, _g(2, 96, 7, 7, 64), kn, dict(MA=2), ("hw_odd", "ks3")),
    ]


RING = {"GEMM_VARIANT": 3, "GEMM_AREG": 0}
AREG = {"GEMM_VARIANT": 3}
TRP = {"GEMM_TR": 2}

CASES = _dword_cases("private", 1) + _dword_cases("lds", 2) + [
    # ---- gemm_i8_dma_kernel, A through LDS (NG = 0): the main loop runs KS - 4 times, then the peeled tail
    _c("r2_ks5_m192_4x5", "ring", _g(2, 160, 4, 5, 192), RING, dict(MA=2, VS=1, MF=1), ("ring_ks5", "hw16_4", "m_full", "spans_images"),
       seeds=(0,) * 7),
    _c("r2_ks4_m176_4x4", "ring", _g(3, 128, 4, 4, 176), RING, dict(MA=2, VS=1), ("ring_ks4", "hw16_0", "m_tail")),
    _c("r2_ks9_m64_7x7", "ring", _g(3, 288, 7, 7, 64), RING, dict(MA=2, MF=1), ("ring_ks_odd", "hw16_1", "hw_odd", "ragged_n")),
    _c("r2_k150_m176_5x6", "ring", _g(2, 150, 5, 6, 176), RING, dict(MA=2), ("ring_ks5", "k_ragged", "hw16_14", "hw_odd")),
    _c("r1_ks4_m96_4x4", "ring", _g(2, 128, 4, 4, 96), RING, dict(MA=1, VS=1, MF=1), ("ring_ks4", "m_full")),
    _c("r1_ks5_m136_4x5", "ring", _g(2, 160, 4, 5, 136), RING, dict(MA=1, VS=1), ("ring_ks5", "m_idle", "m_tail")),
    _c("r1_k270_m32_1x17", "ring", _g(2, 270, 1, 17, 32), RING, dict(MA=1, MF=1), ("ring_ks_odd", "k_ragged", "hw16_1")),
    _c("r1_ks4_m80_7x7", "ring", _g(2, 128, 7, 7, 80), RING, dict(MA=1), ("ring_ks4", "hw_odd")),
    # (GEMM_MA = 1: a layer packed for 64-row wave tiles on 32-row ones)
    _c("r1_ks5_m192_forced", "ring", _g(2, 160, 4, 5, 192), dict(RING, GEMM_MA=1), dict(MA=1, VS=1, MF=1), ("ring_ks5", "ma_forced")),
    # ---- the same kernel with the A fragments in a register ring (NG = KS / 4 groups, straight-line)
    _c("a_ng1_m64_4x4", "areg", _g(2, 128, 4, 4, 64), AREG, dict(MA=2, MF=1, VS=1, NG=1), ("ng1", "hw16_0", "m_full")),
    _c("a_ng1_m64_7x7", "areg", _g(2, 128, 7, 7, 64), AREG, dict(MA=2, MF=1, NG=1), ("ng1", "hw16_1", "hw_odd")),
    _c("a_ng1_m320", "areg", _g(1, 128, 4, 4, 320), AREG, dict(MA=2, MF=1, VS=1, NG=1), ("ng1", "m_idle")),
    _c("a_ng2_m192_4x5", "areg", _g(2, 256, 4, 5, 192), AREG, dict(MA=2, MF=1, VS=1, NG=2), ("ng2", "hw16_4", "spans_images"),
       seeds=(0,) * 7),
    _c("a_ng2_m64_1x17", "areg", _g(2, 256, 1, 17, 64), AREG, dict(MA=2, MF=1, NG=2), ("ng2", "hw16_1")),
    _c("a_ng4_m64_4x4", "areg", _g(3, 512, 4, 4, 64), AREG, dict(MA=2, MF=1, VS=1, NG=4), ("ng4", "ragged_n")),
    _c("a_ng4_m64_5x6", "areg", _g(2, 512, 5, 6, 64), AREG, dict(MA=2, MF=1, NG=4), ("ng4", "hw16_14")),
    _c("a_ng8_m64_4x8", "areg", _g(2, 1024, 4, 8, 64), AREG, dict(MA=2, MF=1, VS=1, NG=8), ("ng8",)),
    _c("a_ng8_m64_7x7", "areg", _g(2, 1024, 7, 7, 64), AREG, dict(MA=2, MF=1, NG=8), ("ng8", "hw_odd")),
    # ---- implicit GEMM on gemm_tr_*: D = 3 K-steps in flight on the 4-wave tiles, 4 on the 8-wave ones (TR_CFG)
    _c("ti_4x1_ks4_ow7", "tr_im", (2, 12, 7, 7, 40, 3, P1, 1, 1, 1), {}, dict(WN=4, WM=1, IM=1), ("tr_ks4", "tr_short", "m_tail")),
    _c("ti_4x1_ks13_ow16", "tr_im", (2, 16, 8, 16, 64, 5, P2, 1, 1, 1), {}, dict(WN=4, WM=1, IM=1), ("tr_d3_long", "tr_rows16", "m_full")),
    _c("ti_2x2_ks5_ow9", "tr_im", (2, 16, 8, 9, 96, 3, P1, 1, 1, 1), {}, dict(WN=2, WM=2, IM=1), ("tr_short",), seeds=(0,) * 7),
    _c("ti_2x2_ks19_s2", "tr_im", (2, 24, 14, 18, 72, 5, P2, 2, 1, 1), {}, dict(WN=2, WM=2, IM=1), ("tr_d3_long", "tr_s2", "tr_short")),
    _c("ti_1x4_ks7_ow20", "tr_im", (2, 24, 5, 20, 136, 3, P1, 1, 1, 1), {}, dict(WN=1, WM=4, IM=1), ("tr_skip", "m_idle")),
    _c("ti_1x4_ks4_ow16", "tr_im", (1, 12, 4, 16, 160, 3, P1, 1, 1, 1), {"TR_CFG": 1}, dict(WN=1, WM=4, IM=1), ("tr_ks4", "tr_rows16")),
    _c("ti_4x2_ks4_ow7", "tr_im", (2, 12, 7, 7, 96, 3, P1, 1, 1, 1), {"TR_CFG": 1}, dict(WN=4, WM=2, IM=1), ("tr_ks4_d4", "tr_short")),
    _c("ti_4x2_ks5_ow16", "tr_im", (2, 16, 8, 16, 128, 3, P1, 1, 1, 1), {"TR_CFG": 0}, dict(WN=4, WM=2, IM=1), ("tr_d4_ks5", "m_full")),
    _c("ti_4x2_ks13_ow20", "tr_im", (2, 16, 6, 20, 72, 5, P2, 1, 1, 1), {"TR_CFG": 1}, dict(WN=4, WM=2, IM=1), ("tr_d4_long", "tr_skip")),
    _c("ti_2x4_ks4_ow9", "tr_im", (2, 12, 8, 9, 136, 3, P1, 1, 1, 1), {"TR_CFG": 2}, dict(WN=2, WM=4, IM=1), ("tr_ks4_d4", "m_idle")),
    _c("ti_2x4_ks5_ow20", "tr_im", (1, 16, 5, 20, 256, 3, P1, 1, 1, 1), {"TR_CFG": 0}, dict(WN=2, WM=4, IM=1), ("tr_d4_ks5", "m_full")),
    _c("ti_2x4_ks19_s2", "tr_im", (2, 24, 9, 22, 200, 5, P2, 2, 1, 1), {"TR_CFG": 2}, dict(WN=2, WM=4, IM=1), ("tr_d4_long", "tr_s2")),
    # ---- plain 1x1 GEMMs on the same kernel (GEMM_TR = 2)
    _c("tp_4x1_ks4_4x4", "tr_plain", _g(2, 128, 4, 4, 64), TRP, dict(WN=4, WM=1), ("tr_ks4", "hw16_0", "m_full")),
    _c("tp_4x1_ks9_7x7", "tr_plain", _g(2, 288, 7, 7, 40), TRP, dict(WN=4, WM=1), ("tr_d3_long", "hw16_1", "hw_odd", "m_tail")),
    _c("tp_2x2_k100_1x17", "tr_plain", _g(2, 100, 1, 17, 96), TRP, dict(WN=2, WM=2), ("tr_ks4", "k_ragged", "hw16_1")),
    _c("tp_2x2_k270_4x5", "tr_plain", _g(2, 270, 4, 5, 128), TRP, dict(WN=2, WM=2), ("tr_d3_long", "hw16_4", "spans_images"),
       seeds=(0,) * 7),
    _c("tp_1x4_ks5_5x6", "tr_plain", _g(2, 160, 5, 6, 136), TRP, dict(WN=1, WM=4), ("hw16_14", "m_idle")),
    _c("tp_1x4_ks4_m256", "tr_plain", _g(1, 128, 4, 4, 256), dict(TRP, GEMM_WIDE=0), dict(WN=1, WM=4), ("tr_ks4", "not_wide")),
    _c("tp_4x2_ks4_7x7", "tr_plain", _g(2, 128, 7, 7, 72), dict(TRP, TR_CFG=1), dict(WN=4, WM=2), ("tr_ks4_d4", "hw_odd")),
    _c("tp_4x2_ks5_4x4", "tr_plain", _g(2, 160, 4, 4, 128), dict(TRP, TR_CFG=0), dict(WN=4, WM=2), ("tr_d4_ks5", "ragged_n")),
    _c("tp_4x2_ks11_4x5", "tr_plain", _g(2, 352, 4, 5, 96), dict(TRP, TR_CFG=1), dict(WN=4, WM=2), ("tr_d4_long",)),
    _c("tp_2x4_ks4_4x5", "tr_plain", _g(2, 128, 4, 5, 136), dict(TRP, TR_CFG=2), dict(WN=2, WM=4), ("tr_ks4_d4", "m_idle")),
    _c("tp_2x4_ks5_7x7", "tr_plain", _g(2, 160, 7, 7, 192), dict(TRP, TR_CFG=0), dict(WN=2, WM=4), ("tr_d4_ks5",)),
    _c("tp_2x4_k340_5x6", "tr_plain", _g(2, 340, 5, 6, 320), dict(TRP, TR_CFG=2), dict(WN=2, WM=4), ("tr_d4_long", "k_ragged")),
    # ---- the wide kernel: every (NTT, K / 32) it is instantiated for; a forced tile lets 32-bit outputs take it too
    _c("w4_ks4_m256_4x4", "wide", _g(2, 128, 4, 4, 256), {"WIDE_NTT": 4}, dict(NTT=4, KS=4), ("hw16_0", "wide_m_full")),
    _c("w4_ks8_m257_4x5", "wide", _g(3, 256, 4, 5, 257), {"WIDE_NTT": 4}, dict(NTT=4, KS=8), ("hw16_4", "wide_m257", "spans_images"),
       seeds=(0,) * 7),
    _c("w4_ks16_m320_1x17", "wide", _g(2, 512, 1, 17, 320), {"WIDE_NTT": 4}, dict(NTT=4, KS=16), ("hw16_1", "wide_m_tail")),
    _c("w4_ks32_m256_5x6", "wide", _g(2, 1024, 5, 6, 256), {"WIDE_NTT": 4}, dict(NTT=4, KS=32), ("hw16_14", "hw_odd")),
    _c("w7_ks4_m320_5x6", "wide", _g(3, 128, 5, 6, 320), {"WIDE_NTT": 7}, dict(NTT=7, KS=4), ("hw16_14", "wide_m_tail")),
    _c("w7_ks8_m256_4x4", "wide", _g(2, 256, 4, 4, 256), {"WIDE_NTT": 7}, dict(NTT=7, KS=8), ("hw16_0",)),
    _c("w7_ks16_m257_4x5", "wide", _g(2, 512, 4, 5, 257), {"WIDE_NTT": 7}, dict(NTT=7, KS=16), ("hw16_4", "wide_m257")),
    _c("w8_ks4_m257_1x17", "wide", _g(2, 128, 1, 17, 257), {"WIDE_NTT": 8}, dict(NTT=8, KS=4), ("hw16_1", "wide_m257")),
    _c("w8_ks8_m256_5x6", "wide", _g(3, 256, 5, 6, 256), {"WIDE_NTT": 8}, dict(NTT=8, KS=8), ("hw16_14", "ragged_n")),
    _c("w8_ks16_m320_4x4", "wide", _g(2, 512, 4, 4, 320), {"WIDE_NTT": 8}, dict(NTT=8, KS=16), ("hw16_0",)),
]
BY_NAME = {c["name"]: c for c in CASES}

# the pointer sweep: per family the cases that also run with x 1 and 3 bytes off a dword and with y 1, 2, 3 elements off its
# vector alignment, on every output kind: (case, what the x-off launch claims, what the y-off launch claims).  Off-dword rows
# take the bytewise loads of the dword kernels (AL = 0) and the scalar stores of both generations; an output off its alignment
# takes the scalar stores alone, which is the only way to (AL 1, VS 0).  tr and wide store row pieces of any alignment.
POINTER_OFFSETS = ((1, 0), (3, 0), (0, 1), (0, 2), (0, 3))
POINTER_CASES = (
    ("p1_ks2_m32", dict(MA=1), dict(MA=1, AL=1)), ("p2_k72_m64", dict(MA=2), dict(MA=2, AL=1)),
    ("l1_ks2_m32", dict(MA=1), dict(MA=1, AL=1)), ("l2_k72_m64", dict(MA=2), dict(MA=2, AL=1)),
    ("r2_ks5_m192_4x5", dict(MA=2, MF=1), dict(MA=2, MF=1)), ("a_ng2_m192_4x5", dict(MA=2, MF=1, NG=2), dict(MA=2, MF=1, NG=2)),
    ("ti_2x2_ks5_ow9", dict(WN=2, WM=2, IM=1), dict(WN=2, WM=2, IM=1)), ("tp_2x2_k270_4x5", dict(WN=2, WM=2), dict(WN=2, WM=2)),
    ("w4_ks8_m257_4x5", dict(NTT=4, KS=8), dict(NTT=4, KS=8)),
)
EDGE_CASES = tuple(c["name"] for c in CASES if c["seeds"])
# batch sweep of distinct images, non-dyadic operands (case, act, alpha) and maximum magnitude (the family's largest K): one per family
BATCH_NS = (1, 2, 3, 9)
BATCH_CASES = ("p1_ks1_7x7", "l2_k100_m48", "r2_ks9_m64_7x7", "a_ng1_m64_7x7", "ti_1x4_ks7_ow20", "tp_1x4_ks5_5x6", "w7_ks4_m320_5x6")
ND_CASES = (("p2_k100_m48", E.ACT_LEAKY, 0.3), ("l1_ks3_m24", E.ACT_RELU6, 5.5), ("r1_ks5_m136_4x5", E.ACT_LEAKY, 0.3),
            ("a_ng4_m64_5x6", E.ACT_RELU, 0.0), ("ti_4x2_ks13_ow20", E.ACT_LEAKY, 0.3), ("tp_2x4_k340_5x6", E.ACT_RELU6, 5.5),
            ("w8_ks8_m256_5x6", E.ACT_LEAKY, 0.3), ("w4_ks16_m320_1x17", E.ACT_RELU6, 5.5))
MAXMAG_CASES = ("p2_k100_m48", "l2_k100_m48", "r2_ks9_m64_7x7", "a_ng8_m64_7x7", "ti_2x4_ks19_s2", "tp_4x2_ks11_4x5", "w4_ks32_m256_5x6")
NEG_ACTS = ((E.ACT_NONE, 0.0), (E.ACT_LEAKY, 0.25), (E.ACT_LEAKY, 0.375))
NN_ACTS = ((E.ACT_RELU, 0.0), (E.ACT_RELU6, 60.0), (E.ACT_RELU6, 60.5), (E.ACT_RELU6, 200.5))


# ---- the plan ------------------------------------------------------------------------------------------------------------
def nonneg(act):
    return int(act in (E.ACT_RELU, E.ACT_RELU6))


def key_of(capi, shape, out, act=E.ACT_NONE, tail=0, n=None):
    """The instance key of the launch of `shape` with output kind `out` under the knobs in force, and the plan's fields."""
    f = T._fields(capi.gemm_plan_text(T.desc_of(capi, shape, n=n), E.OUT_KINDS[out], tail))
    wide = f.get("family") == "wide"
    f["KS"] = shape[1] // 32 if wide else 0
    f["NONNEG"] = nonneg(act) if wide and out == "i8" else 0
    return tuple(f.get(k, 0) for k in KEY_FIELDS), f


def claimed_key(case, out, act=E.ACT_NONE, claim=None):
    """The key a case claims for one launch."""
    c = case["claim"] if claim is None else claim
    fam = {"areg": "ring", "tr_im": "tr", "tr_plain": "tr"}.get(case["family"], case["family"])
    return make_key(fam, out, NONNEG=nonneg(act) if fam == "wide" and out == "i8" else 0, **c)


def mis_tail(mis):
    return (TAIL_X_UNALIGNED if mis[0] else 0) | (TAIL_UNALIGNED if mis[1] else 0)


def acts_of(case):
    """The activations a case runs: E.ACTS with the stated seeds, else one that keeps negative values and one that does not (the
    wide kernel's NONNEG 0 and 1), by the case's place in the table.  [(act, alpha, seed)]."""
    if case["seeds"]:
        return [(a, al, s) for (a, al), s in zip(E.ACTS, case["seeds"])]
    i = CASES.index(case)
    return [NEG_ACTS[i % len(NEG_ACTS)] + (8000 + i,), NN_ACTS[i % len(NN_ACTS)] + (8500 + i,)]


def launches(case):
    """Every launch of a case under aligned pointers: [(out, act, alpha, j)], j the index into acts_of (int32 accumulators run
    once: no epilogue)."""
    acts = acts_of(case)
    return [(out, a, al, j) for out in case["outs"] for j, (a, al, _s) in enumerate(acts) if out != "i32" or j == 0]


def table_keys():
    """Every key the table claims: the cases' launches and the pointer sweep's."""
    keys = {claimed_key(c, out, act) for c in CASES for out, act, _al, _j in launches(c)}
    for name, cx, cy in POINTER_CASES:
        case = BY_NAME[name]
        for out in OUTS:
            for act, _al, _s in acts_of(case)[:2]:
                keys |= {claimed_key(case, out, act, cx), claimed_key(case, out, act, cy)}
    return keys


def _geom(capi, case, f):
    p = dict(f)
    s = case["shape"]
    p["oh"], p["ow"] = capi.out_hw(T.desc_of(capi, s))
    p["n"], p["M"], p["K"], p["stride"] = s[0], s[4], s[1] * s[5] * s[5], s[7]
    p["ksteps"] = -(-p["K"] // 32)
    p["hw"] = p["oh"] * p["ow"]
    p["D"] = p.get("D", 0)
    # columns a block walks and the column space of the batch (gemm_plan: HWP = the 16-byte padded row of ring / tr / wide)
    hwp = (p["HWX"] + 15) & ~15
    p["BN"] = {"tr": p["WN"] * 128, "wide": p["NTT"] * 32}.get(p["family"], 128)
    nb = p["n"] * p["oh"] if p["IM"] else p["n"]
    p["cols"] = nb * (p["HWX"] if p["family"] in ("private", "lds") else hwp)
    p["img_cols"] = p["cols"] // p["n"]
    p["BM"] = {"tr": p["WM"] * 64, "wide": 256}.get(p["family"], 128 * max(p["MA"], 1))
    p["WR"] = {"tr": 64, "wide": 32}.get(p["family"], 32 * max(p["MA"], 1))  # the rows of one wave of the block
    return p


def plan_of(capi, case, out="i8"):
    """The plan of the case's aligned launch with output kind `out` as a dict, the geometry added (under the knobs in force)."""
    return _geom(capi, case, key_of(capi, case["shape"], out)[1])


def _first_gen(p):
    return p["family"] in ("private", "lds", "ring")


def _dword(p):
    return p["family"] in ("private", "lds")


def _end_aligned(p):
    return p["family"] in ("ring", "wide") or (p["family"] == "tr" and p["IM"] == 0)


# class -> predicate on plan_of's dict
CLASSES = {
    # K loop
    "ks1": lambda p: _dword(p) and p["ksteps"] == 1,
    "ks2": lambda p: _dword(p) and p["ksteps"] == 2,
    "ks3": lambda p: _dword(p) and p["ksteps"] == 3,
    "k_ragged": lambda p: p["K"] % 32 != 0,
    "ring_ks4": lambda p: p["family"] == "ring" and p["NG"] == 0 and p["ksteps"] == 4,  # the peeled tail alone
    "ring_ks5": lambda p: p["family"] == "ring" and p["NG"] == 0 and p["ksteps"] == 5,
    "ring_ks_odd": lambda p: p["family"] == "ring" and p["NG"] == 0 and p["ksteps"] >= 9 and p["ksteps"] % 2 == 1,
    "ng1": lambda p: p["NG"] == 1 and p["ksteps"] == 4,
    "ng2": lambda p: p["NG"] == 2 and p["ksteps"] == 8,
    "ng4": lambda p: p["NG"] == 4 and p["ksteps"] == 16,
    "ng8": lambda p: p["NG"] == 8 and p["ksteps"] == 32,
    "tr_ks4": lambda p: p["family"] == "tr" and p["D"] == 3 and p["ksteps"] == 4,      # the minimum, and D + 1
    "tr_d3_long": lambda p: p["family"] == "tr" and p["D"] == 3 and p["ksteps"] >= 9,  # 2 (D + 1) + 1
    "tr_ks4_d4": lambda p: p["family"] == "tr" and p["D"] == 4 and p["ksteps"] == 4,   # fewer K-steps than ring slots
    "tr_d4_ks5": lambda p: p["family"] == "tr" and p["D"] == 4 and p["ksteps"] == 5,
    "tr_d4_long": lambda p: p["family"] == "tr" and p["D"] == 4 and p["ksteps"] >= 11,
    # columns
    "hw16_0": lambda p: _end_aligned(p) and p["hw"] % 16 == 0,
    "hw16_1": lambda p: _end_aligned(p) and p["hw"] % 16 == 1 and p["hw"] > 16,
    "hw16_4": lambda p: _end_aligned(p) and p["hw"] % 16 == 4 and p["hw"] > 16,
    "hw16_14": lambda p: _end_aligned(p) and p["hw"] % 16 == 14 and p["hw"] > 16,
    "hw_odd": lambda p: p["hw"] % 4 != 0 and p["IM"] == 0,
    "hw_quad": lambda p: _dword(p) and p["hw"] % 4 == 0 and p["AL"] == 1,
    "ragged_n": lambda p: p["cols"] % p["BN"] != 0,
    "spans_images": lambda p: p["n"] >= 2 and p["img_cols"] % p["BN"] != 0 and p["cols"] > p["img_cols"],
    "tr_short": lambda p: p["IM"] == 1 and 7 <= p["ow"] < 16,
    "tr_rows16": lambda p: p["IM"] == 1 and p["ow"] == 16,
    "tr_skip": lambda p: p["IM"] == 1 and p["ow"] > 16 and p["ow"] % 16 != 0,
    "tr_s2": lambda p: p["IM"] == 1 and p["stride"] == 2,
    # rows
    "m_tail": lambda p: p["family"] != "wide" and p["M"] % 32 != 0,
    "m_full": lambda p: p["family"] != "wide" and p["M"] % p["BM"] in (0, p["M"]) and p["M"] % (64 if p["family"] == "tr" else 32 * p["MA"]) == 0,
    # a last M block with whole idle waves
    "m_idle": lambda p: p["M"] % p["BM"] != 0 and -(-(p["M"] % p["BM"]) // p["WR"]) < p["BM"] // p["WR"],
    "wide_m257": lambda p: p["family"] == "wide" and p["M"] == 257,
    "wide_m_full": lambda p: p["family"] == "wide" and p["M"] == 256,
    "wide_m_tail": lambda p: p["family"] == "wide" and p["M"] % 256 != 0 and p["M"] % 32 == 0,
    "ma_forced": lambda p: p["family"] == "ring" and p["MA"] == 1 and p["M"] % 64 == 0 and p["M"] > 128,  # (automatic: MA = 2)
    "not_wide": lambda p: p["family"] == "tr" and p["M"] >= 256 and p["K"] in (128, 256, 512, 1024),
}
# the classes every family must have a case in
FAMILY_CLASSES = {
    "private": ("ks1", "ks2", "ks3", "k_ragged", "hw_odd", "hw_quad", "m_tail", "m_full", "m_idle", "ragged_n", "spans_images"),
    "lds": ("ks1", "ks2", "ks3", "k_ragged", "hw_odd", "hw_quad", "m_tail", "m_full", "m_idle", "ragged_n", "spans_images"),
    "ring": ("ring_ks4", "ring_ks5", "ring_ks_odd", "hw16_0", "hw16_1", "hw16_4", "hw16_14", "hw_odd", "m_tail", "m_full", "m_idle",
             "ragged_n", "spans_images"),
    "areg": ("ng1", "ng2", "ng4", "ng8", "hw16_0", "hw16_1", "hw16_4", "hw16_14", "hw_odd", "m_full", "m_idle", "ragged_n", "spans_images"),
    "tr_im": ("tr_ks4", "tr_d3_long", "tr_ks4_d4", "tr_d4_ks5", "tr_d4_long", "tr_short", "tr_rows16", "tr_skip", "tr_s2", "m_tail",
              "m_full", "m_idle"),
    "tr_plain": ("tr_ks4", "tr_d3_long", "tr_ks4_d4", "tr_d4_ks5", "tr_d4_long", "hw16_0", "hw16_1", "hw16_4", "hw16_14", "hw_odd",
                 "m_tail", "m_full", "m_idle", "ragged_n", "spans_images"),
    "wide": ("hw16_0", "hw16_1", "hw16_4", "hw16_14", "hw_odd", "wide_m257", "wide_m_full", "wide_m_tail", "ragged_n", "spans_images"),
}


# ---- the operands --------------------------------------------------------------------------------------------------------
def make(plref, case, act, alpha, seed, n=None, maxmag=False):
    """Operands and the oracle's results of one case (edge_cases.make_case's dict for kind conv)."""
    return E.make_case(plref, T.route_of(case, n), act, alpha, maxmag, seed)


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _reference(plref, name, j):
    act, alpha, seed = acts_of(BY_NAME[name])[j]
    return _freeze(make(plref, BY_NAME[name], act, alpha, seed))


def reference(plref, case, j=0):
    """make() of the case's j-th activation, computed once per process and shared read-only."""
    return _reference(plref, case["name"], j)


def make_nondyadic(plref, case, act, alpha, seed=0):
    """The same shapes with scales that are no powers of two and biases off every grid: what the fp32 epilogue's fused
    multiply-add rounds is then visible."""
    rng = np.random.default_rng([seed, 78, CASES.index(case)])
    n, cin, h, w, cout, k, pads, st, dl, g = case["shape"]
    s = E._plshape(plref, n, cin, h, w, cout, k, k, pads, st, dl, g)
    es, ts = E.channel_plan(cout)
    x = E.activations(rng, (n, cin, h, w))
    wt = E.weights(rng, (cout, cin // g, k, k), (cin // g) * k * k, es, ts)
    acc = plref.conv2d_acc(s, x, wt)
    scale = (rng.uniform(0.55, 0.95, cout) * 2.0 ** -es).astype(np.float32)
    bias = rng.uniform(-40, 40, cout).astype(np.float32)
    return _freeze({"x": x, "w": wt, "acc": acc, "scale": scale, "bias": bias, "act": act, "alpha": alpha,
                    "ref_f32": plref.epilogue(acc, scale, bias, act, alpha, False), "ref_i8": plref.epilogue(acc, scale, bias, act, alpha, True)})


# ---- the edges -----------------------------------------------------------------------------------------------------------
def case_misses(c, act, alpha):
    """Every edge one made case lacks (dwconv_cases' thresholds on edge_cases.edge_stats of the values the int8 output rounds);
    every relu6 bound must be hit, the one above 127 too, and a leaky case needs ties among its negative values."""
    st = E.edge_stats(c["pre"], act, alpha)
    miss = D.stage_misses(st, act, alpha)
    if act == E.ACT_RELU6 and st["clip"] == 0 and "clip" not in miss:
        miss.append("clip")
    if act == E.ACT_LEAKY and leaky_ties(c) == 0:
        miss.append("leaky_tie")
    return miss


def leaky_ties(c):
    """Negative pre-activation values whose product with alpha is an exact tie (the values are the oracle's)."""
    f = np.asarray(c["pre"], np.float64).ravel()
    return int(((f < 0) & (np.abs(f - np.trunc(f)) == 0.5)).sum())


def find_seeds(plref, case, limit=400):
    """The first seed per activation of E.ACTS at which the oracle's results of `case` lack no edge (how the table's seeds were
    chosen; None where `limit` seeds do not do)."""
    return tuple(next((s for s in range(limit) if not case_misses(make(plref, case, a, al, s), a, al)), None) for a, al in E.ACTS)
