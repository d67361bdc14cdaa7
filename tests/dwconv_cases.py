"""Fusion G (plhip_dw_conv1x1_fused_int8) on every branch of its launch plan: the case table, the class predicates read off the
library's own plan text, and the operands (used by test_gpu_dwconv_envelope.py and its CPU guard test_dwconv_cases.py).

A case is (n, C, h, w, stride, pads (t, b, l, r), M), the smallest shape that reaches a regime of dw_conv1x1_launch_plan
(csrc/dw_plan.h); the class it claims is a predicate on capi.dw_plan_text, so a plan change that moves a case out of its regime
fails on the host.  The operands are edge_cases' two-stage construction (dyadic folded scales, quarter biases, one output of
every channel pinned to an anchor), and the tail adds a residual in quarters and a calib scale of 1/2: the int8 outputs of the
depthwise stage, of the 1x1 stage and of the calib copy sit on exact ties and past both saturation bounds.  The cases with
`seeds` state the seeds at which the oracle alone shows every one of those edges (test_dwconv_cases.py counts them).

The reference is always plref, in the order of the instructions the launch replaces: depthwise conv2d_acc + epilogue (int8),
1x1 conv2d_acc + epilogue, elementwise_add, calib_f32_to_i8.  No device code here."""
import functools

import numpy as np

import edge_cases as E

P1, P0 = (1, 1, 1, 1), (0, 0, 0, 0)


def _c(name, group, shape, classes, seeds=None, x_off=0):
    """seeds: one per activation pair of EDGE_ACTS, searched (find_seeds) so that the oracle's results reach every edge."""
    return {"name": name, "group": group, "shape": shape, "classes": tuple(classes), "seeds": seeds, "x_off": x_off}


# the activations of a case with stated seeds: (1x1 NONE, depthwise relu6 60.5) and (1x1 relu6 60, depthwise NONE) -- between
# them each stage has ties of both signs, both saturation bounds and a relu6 bound (edge_cases.DW_ACTS pairs them)
EDGE_ACTS = ((E.ACT_NONE, 0.0), (E.ACT_RELU6, 60.0))

CASES = [
    # rows wider than 128 outputs: 128-column segments with real left neighbours (ixb = cx0 S - 4), the last one ragged
    _c("wide130", "wide", (2, 16, 3, 130, 1, P1, 8), ("wide", "wide_ragged", "bytes", "tpi6"), seeds=(0, 0)),
    _c("wide256", "wide", (1, 16, 2, 256, 1, P1, 8), ("wide", "wide_exact", "dword")),
    # stride 2 at CW = 128: WP = 264, 66 dwords per row: a second trip of the staging loop
    _c("s2_wide130", "s2wide", (1, 16, 4, 260, 2, P1, 8), ("wide", "wide_ragged", "s2", "pl1", "wu66")),
    _c("s2_wide256_pl0", "s2wide", (1, 16, 4, 512, 2, (0, 1, 0, 1), 8), ("wide", "wide_exact", "s2", "pl0", "wu66"), seeds=(1, 0)),
    _c("s2_128", "s2wide", (1, 16, 4, 256, 2, P1, 8), ("one_segment", "s2", "pl1", "wu66")),
    # TR halved by the LDS loop: narrow, tall planes
    _c("halved_s2_ow4", "halved", (1, 16, 66, 8, 2, P1, 8), ("halved", "ragged_rows", "dword"), seeds=(1, 0)),
    _c("halved_s2_ow5", "halved", (1, 16, 52, 10, 2, P1, 8), ("halved", "bytes")),
    _c("halved_s1_ow1", "halved", (1, 16, 140, 1, 1, P1, 8), ("halved", "ragged_rows", "cw1")),
    # a ragged last M group (mt32 % mtpb != 0), with an M tail in the last tile / without
    _c("ragged_m264", "ragged_m", (1, 32, 14, 14, 1, P1, 264), ("ragged_mgroup", "m_tail", "nacc8"), seeds=(0, 0)),
    _c("ragged_m544", "ragged_m", (1, 32, 7, 7, 1, P1, 544), ("ragged_mgroup", "nacc8")),
    # accumulators per wave, and four whole M groups
    _c("nacc1_m32", "nacc", (1, 16, 14, 14, 1, P1, 32), ("nacc1",)),
    _c("nacc2_m64", "nacc", (1, 16, 14, 14, 1, P1, 64), ("nacc2",)),
    _c("nacc4_m128", "nacc", (1, 16, 14, 14, 1, P1, 128), ("nacc4",)),
    _c("nacc8_m256", "nacc", (1, 16, 14, 14, 1, P1, 256), ("nacc8",)),
    _c("nacc8_m1024", "nacc", (1, 16, 14, 14, 1, P1, 1024), ("nacc8", "mgroups4")),
    # one-pixel outputs
    _c("pixel_pad", "pixel", (1, 16, 1, 1, 1, P1, 8), ("one_pixel",)),
    _c("pixel_s2", "pixel", (1, 16, 3, 3, 2, P0, 8), ("one_pixel", "s2", "pl0")),
    # K-steps: half-filled, full, odd count (buffer parity), the maximum
    _c("k16", "ksteps", (2, 16, 3, 3, 1, P1, 8), ("ks1", "half_kstep")),
    _c("k32", "ksteps", (2, 32, 3, 3, 1, P1, 8), ("ks1", "full_kstep")),
    _c("k48", "ksteps", (2, 48, 3, 3, 1, P1, 8), ("ks2", "half_kstep")),
    _c("k96", "ksteps", (2, 96, 3, 3, 1, P1, 8), ("ks3", "full_kstep")),
    _c("k1024", "ksteps", (2, 1024, 3, 3, 1, P1, 8), ("ks32", "full_kstep")),
    # x off its 4-byte alignment while w % 4 == 0: rows staged byte by byte because of the pointer
    _c("x_aligned_8x8", "x_misaligned", (2, 16, 8, 8, 1, P1, 8), ("dword", "tpi1"), seeds=(0, 0)),
]
CASES += [_c("x_off%d_8x8" % o, "x_misaligned", (2, 16, 8, 8, 1, P1, 8), ("x_misaligned",), x_off=o) for o in (1, 2, 3)]
CASES += [_c("x_off%d_wide256" % o, "x_misaligned", (1, 16, 2, 256, 1, P1, 8), ("x_misaligned", "wide"), x_off=o) for o in (1, 2, 3)]
# every padding combination on both strides, a plane wider than tall and one taller than wide
CASES += [_c("pad%d%d%d%d_s%d_%dx%d" % (t, b, l, r, s, h, w), "pads", (2, 16, h, w, s, (t, b, l, r), 8), ("s%d" % s, "pl%d" % l))
          for (h, w) in ((5, 6), (6, 5)) for s in (1, 2) for t in (0, 1) for b in (0, 1) for l in (0, 1) for r in (0, 1)]
BY_NAME = {c["name"]: c for c in CASES}
GROUPS = tuple(dict.fromkeys(c["group"] for c in CASES))
EDGE_CASES = tuple(c["name"] for c in CASES if c["seeds"])
# the graph tail runs on these (fp32 sum kept and dropped, residual with and without relu, calib copy alone)
TAILS = {"calib": (False, False), "res": (True, False), "res_relu": (True, True)}
CALIB = 0.5
# batch: distinct images on a tpi > 1 plan (blockIdx.x / tpi by the magic number) and on a tpi == 1 plan
BATCH_CASES, BATCH_NS = ("wide130", "x_aligned_8x8"), (1, 2, 3, 9)


# ---- the plan ------------------------------------------------------------------------------------------------------------
def parse_plan(text):
    """The plan text as a dict: name, the K=V fields as ints (those behind '|', the argument block's, win: KS), grid as a pair."""
    f = {"name": text.split(" ")[0], "text": text}
    for tok in text.split(" ")[1:]:
        k, eq, v = tok.partition("=")
        if not eq:
            continue
        if k == "grid":
            f[k] = tuple(int(t) for t in v.split(","))
        elif k not in ("div", "why"):
            f[k] = int(v)
    return f


def desc_of(capi, shape, act=E.ACT_NONE, alpha=0.0, n=None):
    n0, c, h, w, st, pads, _m = shape
    return capi.conv_desc(n0 if n is None else n, c, h, w, c, 3, 3, pads, (st, st), (1, 1), c, act, alpha)


def plan_of(capi, case, out="f32", has_tail=0, x_aligned=None):
    """The library's launch plan of the case (x aligned unless the case offsets it), with the output plane added."""
    if x_aligned is None:
        x_aligned = int(case["x_off"] % 4 == 0)
    d = desc_of(capi, case["shape"])
    p = parse_plan(capi.dw_plan_text(d, capi.DW_PLAN_PAIR_G, case["shape"][6], E.OUT_KINDS[out], has_tail, x_aligned))
    p["oh"], p["ow"] = capi.out_hw(d)
    p["M"], p["C"] = case["shape"][6], case["shape"][1]
    return p


def _first_tr(p):
    return min(128 // p["ow"], p["oh"]) if p["ow"] <= 128 else 1


# class -> predicate on plan_of's dict
CLASSES = {
    "wide": lambda p: p["cw_tiles"] > 1 and p["CW"] == 128 and p["TR"] == 1 and p["ow"] > 128,
    "wide_ragged": lambda p: p["cw_tiles"] == 2 and p["ow"] % 128 != 0,
    "wide_exact": lambda p: p["cw_tiles"] == 2 and p["ow"] == 256,
    "one_segment": lambda p: p["cw_tiles"] == 1 and p["CW"] == 128 and p["ow"] == 128,
    "bytes": lambda p: p["DWORD"] == 0 and p["wu"] == p["WP"],
    "dword": lambda p: p["DWORD"] == 1 and p["wu"] * 4 == p["WP"],
    "tpi6": lambda p: p["tr_tiles"] == 3 and p["tpi"] == 6,
    "tpi1": lambda p: p["tpi"] == 1,
    "s1": lambda p: p["S"] == 1,
    "s2": lambda p: p["S"] == 2,
    "pl0": lambda p: p["PL"] == 0,
    "pl1": lambda p: p["PL"] == 1,
    "wu66": lambda p: p["DWORD"] == 1 and p["WP"] == 264 and p["wu"] == 66 and p["rpp"] == 1,
    "halved": lambda p: p["ow"] <= 128 and p["TR"] < _first_tr(p) and p["TR"] == (_first_tr(p) + 1) // 2,
    "ragged_rows": lambda p: p["tr_tiles"] > 1 and p["oh"] % p["TR"] != 0,
    "cw1": lambda p: p["CW"] == 1 and p["ow"] == 1,
    "ragged_mgroup": lambda p: p["mgroups"] > 1 and p["mt32"] % p["mtpb"] != 0 and p["grid"][1] == p["mgroups"],
    "m_tail": lambda p: p["M"] % 32 != 0,
    "nacc1": lambda p: p["NACC"] == 1,
    "nacc2": lambda p: p["NACC"] == 2,
    "nacc4": lambda p: p["NACC"] == 4,
    "nacc8": lambda p: p["NACC"] == 8,
    "mgroups4": lambda p: p["mgroups"] == 4 and p["mt32"] % p["mtpb"] == 0,
    "one_pixel": lambda p: p["oh"] == 1 and p["ow"] == 1,
    "ks1": lambda p: p["KS"] == 1,
    "ks2": lambda p: p["KS"] == 2,
    "ks3": lambda p: p["KS"] == 3,
    "ks32": lambda p: p["KS"] == 32,
    "half_kstep": lambda p: p["C"] % 32 == 16,
    "full_kstep": lambda p: p["C"] % 32 == 0,
    "x_misaligned": lambda p: p["DWORD"] == 0,  # (and the aligned plan of the same shape stages dwords: test_dwconv_cases.py)
}


# ---- the operands --------------------------------------------------------------------------------------------------------
def route_of(case, n=None):
    """The case as a row of edge_cases.ROUTES (kind dwconv), at batch n."""
    n0, c, h, w, st, pads, m = case["shape"]
    return E._r(case["name"], "dwconv", (n0 if n is None else n, c, h, w, c, 3, 3, pads, st, 1, c), m=m, kernel="dw_conv1x1")


def acts_of(case):
    """The 1x1 stage's activations a case runs: EDGE_ACTS with the stated seeds, else one of edge_cases.ACTS by the case's
    place in the table.  [(act, alpha, seed)]."""
    if case["seeds"]:
        return [(a, al, s) for (a, al), s in zip(EDGE_ACTS, case["seeds"])]
    i = CASES.index(case)
    return [E.ACTS[i % len(E.ACTS)] + (5000 + i,)]


def add_tail(plref, c, seed):
    """A residual in quarters and the calib scale 1/2 for every tail of TAILS: z (the fp32 sum), q (the calib copy) and pre_q
    (the value the calib copy rounds: 2 z, exact)."""
    rng = np.random.default_rng([seed, 1])
    res = (np.round(rng.uniform(-70, 70, c["pre"].shape) * 4) / 4).astype(np.float32)
    c["res"], c["calib"], c["tails"] = res, CALIB, {}
    for key, (use_res, relu) in TAILS.items():
        z = plref.elementwise_add(c["pre"], res, relu) if use_res else c["pre"]
        c["tails"][key] = {"res": res if use_res else None, "relu": relu, "z": z, "q": plref.calib_f32_to_i8(z, CALIB),
                           "pre_q": (z.astype(np.float64) / CALIB).astype(np.float32)}
    return c


def make(plref, case, act, alpha, seed, n=None):
    """Operands and the oracle's results of one case (edge_cases.make_case's dict for kind dwconv, plus the tails)."""
    return add_tail(plref, E.make_case(plref, route_of(case, n), act, alpha, False, seed), seed)


@functools.lru_cache(maxsize=None)
def _reference(plref, name, j):
    act, alpha, seed = acts_of(BY_NAME[name])[j]
    c = make(plref, BY_NAME[name], act, alpha, seed)
    for v in list(c.values()) + [a for t in c["tails"].values() for a in t.values()]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def reference(plref, case, j=0):
    """make() of the case's j-th activation, computed once per process and shared read-only."""
    return _reference(plref, case["name"], j)


# ---- the edges -----------------------------------------------------------------------------------------------------------
def stage_misses(st, act, alpha):
    """What a conv stage's pre-rounding values (edge_cases.edge_stats) lack of the edges its activation admits: [] when it has
    ties of every sign the activation lets through, both (or the positive) saturation bounds with a value exactly on +-127.5,
    the relu6 bound where that lies inside the int8 range, and fractions that tell round-toward-zero from nearest-even."""
    n, miss = st["n"], []
    if st["tie_pos"] < 0.01 * n:
        miss.append("tie_pos")
    if act in (E.ACT_NONE, E.ACT_LEAKY):
        miss += [k for k in ("tie_neg",) if st[k] < 0.01 * n] + [k for k in ("sat_neg",) if st[k] == 0]
    if act == E.ACT_NONE and st["at_m127_5"] == 0:
        miss.append("at_m127_5")
    if act == E.ACT_RELU6 and alpha < 127:
        miss += [k for k in ("clip",) if st[k] == 0]
    else:
        miss += [k for k in ("sat_pos", "at_127_5") if st[k] == 0]
    if st["rtz"] == 0:
        miss.append("rtz")
    return miss


def calib_misses(t, key, act, alpha):
    """The same for a calib copy (pre_q = z / calib scale).  A sum with a residual reaches both signs unless it goes through a
    relu; the calib copy of the 1x1 output alone reaches what that output's activation lets through, and under relu6 the bound
    itself (2 alpha)."""
    st = E.edge_stats(t["pre_q"], E.ACT_RELU6 if key == "calib" else E.ACT_NONE, alpha / CALIB)
    n = st["n"]
    nonneg = t["relu"] or (key == "calib" and act in (E.ACT_RELU, E.ACT_RELU6))
    miss = [k for k in ("tie_pos",) + (() if nonneg else ("tie_neg",)) if st[k] < 0.01 * n]
    if key == "calib" and act == E.ACT_RELU6 and alpha / CALIB < 127:
        miss += [k for k in ("clip",) if st[k] == 0]
    else:
        miss += [k for k in ("sat_pos",) + (() if nonneg else ("sat_neg",)) if st[k] == 0]
    if st["rtz"] == 0:
        miss.append("rtz")
    return miss


def case_misses(c, act, alpha):
    """Every edge one made case lacks, over the depthwise stage, the 1x1 stage and the three calib copies."""
    miss = ["dw:" + m for m in stage_misses(E.edge_stats(c["pre_mid"], c["dw_act"], c["dw_alpha"]), c["dw_act"], c["dw_alpha"])]
    miss += ["pw:" + m for m in stage_misses(E.edge_stats(c["pre"], act, alpha), act, alpha)]
    for key, t in c["tails"].items():
        miss += ["%s:%s" % (key, m) for m in calib_misses(t, key, act, alpha)]
    return miss


def find_seeds(plref, case, limit=400):
    """The first seed per activation of EDGE_ACTS at which the oracle's results of `case` lack no edge (how the table's seeds
    were chosen; None where `limit` seeds do not do)."""
    found = []
    for act, alpha in EDGE_ACTS:
        found.append(next((s for s in range(limit) if not case_misses(make(plref, case, act, alpha, s), act, alpha)), None))
    return tuple(found)
