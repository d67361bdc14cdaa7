"""The fused conv tail (plhip_conv2d_int8_fused) on every kernel and store path that takes it: the case table, the instance each
case claims read off the library's own plan text, and the operands (used by test_gpu_conv_tail.py and its CPU guard
test_tail_cases.py).  The pattern is dwconv_cases.py's.

A case is (n, cin, h, w, cout, k, pads (t, b, l, r), stride, dilation, groups), the smallest shape that reaches one kernel
instance behind a route whose kRoutes row sets fused_tail (csrc/plhip_capi_conv.hip).  `impl` is the route
(plhip_conv_impl_name), `kernel` the instance: the GEMM plan's name (capi.gemm_plan_text, with the tail bits), the patch plan's
launcher and mode (capi.patch_plan_text), "stem7x7s2" for the 7x7 stem; the im2col route's instances carry its group count.
`classes` are predicates on the plan, so a threshold that moves a case out of its store path fails on the host.

The tail is written five times over; `family` says which of them a case runs:
  gemm    gemm_epilogue (gemm_epilogue.h): gemm_nchw, gemm_vperm_lds, gemm_ring, gemm_ring_ma1, gemm_areg, the 7x7 stem
  tr      the 32-bit epilogue of gemm_tr_i8.hip, and tr_stage_i8_calib when the tail is "calib, fp32 dropped, no residual"
  patch   the 32-bit epilogue of conv_patch_kernel.h, local and global mode
  groups  gemm_epilogue behind run_gemm_groups' per-group offsets of y, the residual and the int8 copy (im2col route)

What the table cannot hold, read off conv_patch_supported: the 2 x 2 wave layout (patch_stat_b, cout <= 64) exists for cin == 64
only and not in global mode, so "patch_stat_b at three chunks" and "patch_stat_b global" are shapes the route declines (they
land on gemm_tr_4x1); the guard test asserts that they do.

Operands are edge_cases' construction (dyadic folded scales, quarter biases, one output of every channel on an anchor) with
dwconv_cases.add_tail's residual in quarters and calib scale 1/2: the calib copy sits on exact ties of both signs and past both
saturation bounds.  The reference is always plref in the order of the instructions the launch replaces: conv2d_acc + epilogue,
elementwise_add, calib_f32_to_i8.  No device code here."""
import functools

import numpy as np

import dwconv_cases as D
import edge_cases as E

P0, P1, P2, P3 = (0,) * 4, (1,) * 4, (2,) * 4, (3,) * 4
GEMM, STEM = "conv1x1s1_gemm_int8_mfma32x32x32", "conv_7x7s2_direct_int8_mfma32x32x32"
IMPLICIT, IM2COL = "conv_implicit_gemm_int8_mfma32x32x32", "conv_im2col_gemm_int8_mfma32x32x32"
PATCH, PATCH_S2 = "conv_patch_gemm_int8_mfma32x32x32", "conv_patch_s2_gemm_int8_mfma32x32x32"
DIRECT_S2 = "conv_3x3s2_direct_int8_mfma32x32x32"
TAIL_RES, TAIL_CALIB, TAIL_NO_F32, TAIL_UNALIGNED = 1, 2, 4, 8  # capi.TAIL_*


def _c(name, family, shape, impl, kernel, classes=(), seeds=None):
    """seeds: one per activation of EDGE_ACTS, searched (find_seeds) so that the oracle's results reach every edge."""
    return {"name": name, "family": family, "shape": shape, "impl": impl, "kernel": kernel, "classes": tuple(classes), "seeds": seeds}


# the activations of a case with stated seeds: between them the calib copy of gemm_epilogue takes round_sat_i8 (NONE) and the
# packed non-negative path (relu6), and the conv output has ties of both signs, both saturation bounds and a relu6 bound
EDGE_ACTS = ((E.ACT_NONE, 0.0), (E.ACT_RELU6, 60.0))

CASES = [
    # ---- gemm_epilogue: the first-generation GEMM kernels on the NCHW slab
    _c("nchw_7x7", "gemm", (2, 16, 7, 7, 24, 1, P0, 1, 1, 1), GEMM, "gemm_nchw", ("vs0", "al0", "m_tail"), seeds=(0, 0)),
    _c("nchw_4x8", "gemm", (2, 32, 4, 8, 24, 1, P0, 1, 1, 1), GEMM, "gemm_nchw", ("vs1", "m_tail")),
    _c("lds_6x6", "gemm", (2, 64, 6, 6, 96, 1, P0, 1, 1, 1), GEMM, "gemm_vperm_lds", ("vs1", "m_full"), seeds=(0, 0)),
    _c("lds_m80", "gemm", (2, 64, 6, 6, 80, 1, P0, 1, 1, 1), GEMM, "gemm_vperm_lds", ("vs1", "m_tail")),
    _c("ring_4x5", "gemm", (2, 160, 4, 5, 256, 1, P0, 1, 1, 1), GEMM, "gemm_ring", ("vs1", "m_full", "ks5"), seeds=(0, 0)),
    _c("ring_ma1_4x5", "gemm", (2, 256, 4, 5, 200, 1, P0, 1, 1, 1), GEMM, "gemm_ring_ma1", ("vs1", "m_tail")),
    _c("areg_4x8", "gemm", (2, 128, 4, 8, 256, 1, P0, 1, 1, 1), GEMM, "gemm_areg", ("vs1", "m_full", "wide_eligible")),
    # the end-aligned last piece of a 49-column image: skip != 0, the residual read through the i >= skip filter
    _c("ring_7x7", "gemm", (2, 160, 7, 7, 256, 1, P0, 1, 1, 1), GEMM, "gemm_ring", ("vs0", "ring_skip"), seeds=(0, 0)),
    _c("ring_ma1_7x7", "gemm", (2, 256, 7, 7, 200, 1, P0, 1, 1, 1), GEMM, "gemm_ring_ma1", ("vs0", "ring_skip", "m_tail")),
    _c("areg_7x7", "gemm", (2, 128, 7, 7, 256, 1, P0, 1, 1, 1), GEMM, "gemm_areg", ("vs0", "ring_skip")),
    # ---- the 7x7 stride-2 stem (gemm_epilogue through conv_stem_common.h)
    _c("stem_m64", "gemm", (1, 3, 20, 32, 64, 7, P3, 2, 1, 1), STEM, "stem7x7s2", (), seeds=(0, 0)),
    _c("stem_m40", "gemm", (1, 3, 20, 32, 40, 7, P3, 2, 1, 1), STEM, "stem7x7s2", ()),
    # ---- implicit GEMM on gemm_tr_*: 3x3 / 5x5 with cin 16 / 24 (the patch route declines), one block shape per M range
    _c("tr_m48_ow16", "tr", (2, 16, 8, 16, 48, 3, P1, 1, 1, 1), IMPLICIT, "gemm_tr_4x1", ("tr_rows16", "out_flip"), seeds=(0, 0)),
    _c("tr_m40_ow7", "tr", (2, 16, 7, 7, 40, 3, P1, 1, 1, 1), IMPLICIT, "gemm_tr_4x1", ("tr_short", "out_flip")),
    _c("tr_m96_ow9", "tr", (2, 16, 8, 9, 96, 3, P1, 1, 1, 1), IMPLICIT, "gemm_tr_2x2", ("tr_short", "out_flip"), seeds=(0, 0)),
    _c("tr_m128_ow16", "tr", (2, 24, 9, 16, 128, 5, P2, 1, 1, 1), IMPLICIT, "gemm_tr_2x2", ("tr_rows16", "out_flip")),
    _c("tr_m136_ow11", "tr", (2, 24, 9, 11, 136, 5, P2, 1, 1, 1), IMPLICIT, "gemm_tr_1x4", ("tr_short", "out_flip")),
    _c("tr_m160_ow20", "tr", (2, 24, 5, 20, 160, 3, P1, 1, 1, 1), IMPLICIT, "gemm_tr_1x4", ("tr_skip", "out_flip")),
    _c("tr_s2_ow9", "tr", (2, 16, 14, 18, 72, 3, P1, 2, 1, 1), IMPLICIT, "gemm_tr_2x2", ("tr_short", "tr_s2", "out_flip")),
    # ---- im2col: run_gemm_groups advances y, the residual and the int8 copy per group; the 1x1 stride-2 subsample
    _c("im2col_g2_dil2", "groups", (2, 16, 11, 11, 48, 3, P2, 1, 2, 2), IM2COL, "im2col_g2/gemm_nchw", ("vs0", "pad_columns"), seeds=(0, 0)),
    _c("subsample_s2", "groups", (2, 48, 10, 12, 64, 1, P0, 2, 1, 1), IM2COL, "im2col_g1/gemm_nchw", ("vs0", "pad_columns")),
    # ---- the patch kernel: the three stride-1 launchers and the stride-2 form, local and global mode
    _c("stat_a_14", "patch", (2, 64, 6, 14, 96, 3, P1, 1, 1, 1), PATCH, "patch_stat_a/local", ("ragged_ow",), seeds=(0, 0)),
    _c("stat_a_m65_13", "patch", (2, 64, 5, 13, 65, 3, P1, 1, 1, 1), PATCH, "patch_stat_a/local", ("patch_m_tail", "ragged_ow")),
    _c("stat_b_m64", "patch", (2, 64, 6, 14, 64, 3, P1, 1, 1, 1), PATCH, "patch_stat_b/local", ("chunks2", "ragged_ow")),
    _c("stat_b_m40", "patch", (2, 64, 6, 12, 40, 3, P1, 1, 1, 1), PATCH, "patch_stat_b/local", ("chunks2", "patch_m_tail", "whole_ow")),
    _c("stream_a_14", "patch", (2, 96, 6, 14, 96, 3, P1, 1, 1, 1), PATCH, "patch_stream_a/local", ("chunks3", "ragged_ow")),
    _c("s2_18", "patch", (2, 64, 10, 18, 96, 3, P1, 2, 1, 1), PATCH_S2, "patch_s2/local", ("ragged_ow",)),
    # a 7-wide plane: global mode; batch 3, so that the one tile spans the images
    _c("stat_a_7x7", "patch", (3, 64, 7, 7, 96, 3, P1, 1, 1, 1), PATCH, "patch_stat_a/global", ("spans_images", "ragged_ow"), seeds=(0, 0)),
    _c("stream_a_7x7", "patch", (3, 96, 7, 7, 96, 3, P1, 1, 1, 1), PATCH, "patch_stream_a/global", ("spans_images", "chunks3")),
    _c("s2_7x7_m65", "patch", (3, 32, 13, 13, 65, 3, P1, 2, 1, 1), PATCH_S2, "patch_s2/global", ("spans_images", "patch_m_tail"),
       seeds=(0, 0)),
]
BY_NAME = {c["name"]: c for c in CASES}
FAMILIES = ("gemm", "tr", "patch", "groups")
EDGE_CASES = tuple(c["name"] for c in CASES if c["seeds"])
# every instance a tail launch can reach under default knobs (test_tail_cases.py holds the table to exactly this set)
INSTANCES = {
    "gemm_nchw", "gemm_vperm_lds", "gemm_ring", "gemm_ring_ma1", "gemm_areg",
    "gemm_tr_4x1", "gemm_tr_2x2", "gemm_tr_1x4",
    "patch_stat_a/local", "patch_stat_a/global", "patch_stat_b/local", "patch_stream_a/local", "patch_stream_a/global",
    "patch_s2/local", "patch_s2/global",
    "stem7x7s2", "im2col_g2/gemm_nchw", "im2col_g1/gemm_nchw",
}
# shapes the issue's list names that the patch route declines (conv_patch_supported): (shape, where they land)
DECLINED = (((2, 96, 6, 14, 64, 3, P1, 1, 1, 1), "gemm_tr_4x1"), ((3, 64, 7, 7, 64, 3, P1, 1, 1, 1), "gemm_tr_4x1"))
# a tail on this one is refused: the direct 3x3 stride-2 stem has none
REFUSED_SHAPE = (2, 3, 16, 16, 40, 3, P1, 2, 1, 1)
# the graph tails: key -> (residual, relu behind it, calib copy).  Each calib tail runs with the fp32 sum kept and dropped.
TAILS = {"calib": (False, False, True), "res": (True, False, True), "res_relu": (True, True, True), "res_relu_f32": (True, True, False)}
CALIB = D.CALIB
# batch sweep: a GEMM plan, the global-mode patch plan, an implicit gemm_tr plan
BATCH_CASES, BATCH_NS = ("ring_7x7", "stat_a_7x7", "tr_m96_ow9"), (1, 2, 3, 9)
# non-dyadic operand sets, one or two per family: (case, act, alpha).  Calib scale 0.3: the kernel's multiply by 1 / scale.
ND_CALIB = 0.3
ND_CASES = (("lds_m80", E.ACT_LEAKY, 0.3), ("areg_7x7", E.ACT_RELU, 0.0), ("stem_m40", E.ACT_RELU6, 5.5),
            ("tr_m136_ow11", E.ACT_LEAKY, 0.3), ("tr_m160_ow20", E.ACT_RELU, 0.0),
            ("stat_a_m65_13", E.ACT_LEAKY, 0.3), ("s2_7x7_m65", E.ACT_NONE, 0.0), ("im2col_g2_dil2", E.ACT_LEAKY, 0.3))


# ---- the plan ------------------------------------------------------------------------------------------------------------
def desc_of(capi, shape, act=E.ACT_NONE, alpha=0.0, n=None):
    n0, cin, h, w, cout, k, pads, st, dl, g = shape
    return capi.conv_desc(n0 if n is None else n, cin, h, w, cout, k, k, pads, (st, st), (dl, dl), g, act, alpha)


def _fields(text):
    f = {"name": text.split(" ")[0], "text": text}
    for tok in text.split(" ")[1:]:
        k, _eq, v = tok.partition("=")
        f[k] = int(v) if v.lstrip("-").isdigit() else v
    return f


def plan_of(capi, shape, tail=TAIL_RES | TAIL_CALIB, n=None):
    """The launch plan of a tail launch on `shape` as a dict: impl, kernel (the instance, as the table spells it) and the fields
    of the library's plan text; the geometry (oh, ow, M, groups) added."""
    import ctypes
    d = desc_of(capi, shape, n=n)
    impl = capi.load().plhip_conv_impl_name(ctypes.byref(d)).decode()
    p = {"impl": impl, "family": "", "text": ""}
    gt, pt = capi.gemm_plan_text(d, E.OUT_KINDS["f32"], tail), capi.patch_plan_text(d)
    if gt:
        p.update(_fields(gt))
        p["kernel"] = ("im2col_g%d/" % shape[9] if impl == IM2COL else "") + p["name"]
    elif pt:
        p.update(_fields(pt))
        p["kernel"] = "%s/%s" % (p["name"], "global" if p["glob"] else "local")
    else:
        p["kernel"] = "stem7x7s2" if impl == STEM else impl
    p["oh"], p["ow"] = capi.out_hw(d)
    p["M"], p["groups"], p["stride"] = shape[4], shape[9], shape[7]
    return p


def _first_gen(p):
    return p["family"] in ("private", "lds", "ring")


# class -> predicate on plan_of's dict (the plan of the tail "residual + calib", aligned pointers)
CLASSES = {
    "vs0": lambda p: _first_gen(p) and p["VS"] == 0,
    "vs1": lambda p: _first_gen(p) and p["VS"] == 1,
    "al0": lambda p: p["family"] == "private" and p["AL"] == 0 and p["ow"] * p["oh"] % 4 != 0,
    "m_tail": lambda p: _first_gen(p) and (p["M"] // p["groups"]) % (32 * p["MA"]) != 0 and p["MF"] == 0,
    "m_full": lambda p: _first_gen(p) and p["M"] % (32 * p["MA"]) == 0 and p["MF"] == 1,
    "ks5": lambda p: p["family"] == "ring" and p["NG"] == 0 and p["MA"] == 2,
    "ring_skip": lambda p: p["family"] == "ring" and p["HWX"] % 16 != 0 and p["HWX"] % 4 != 0 and p["HWX"] > 16,
    "wide_eligible": lambda p: p["family"] == "ring",  # (and gemm_wide_* without a tail: test_tail_cases.py)
    "tr_rows16": lambda p: p["family"] == "tr" and p["IM"] == 1 and p["HWX"] == 16,
    "tr_skip": lambda p: p["family"] == "tr" and p["IM"] == 1 and p["HWX"] > 16 and p["HWX"] % 16 != 0,
    "tr_short": lambda p: p["family"] == "tr" and p["IM"] == 1 and 7 <= p["HWX"] <= 15,
    "tr_s2": lambda p: p["family"] == "tr" and p["stride"] == 2,
    "out_flip": lambda p: p["family"] == "tr" and p["OUT"] == E.OUT_KINDS["f32"],  # (flipped by one tail word only: the guard)
    "ragged_ow": lambda p: "patch" in p["name"] and p["OW"] % 4 != 0,
    "whole_ow": lambda p: "patch" in p["name"] and p["OW"] % 4 == 0,
    "patch_m_tail": lambda p: "patch" in p["name"] and p["M"] % 32 != 0,
    "chunks2": lambda p: p["name"] == "patch_stat_b" and p["NCH"] == 2,
    "chunks3": lambda p: p["name"] == "patch_stream_a" and p["NCH"] == 3,
    # global mode: one "image" of all the images' pixels, and fewer tiles than images, so a tile spans images
    "spans_images": lambda p: p["glob"] == 1 and p["B"] == 1 and p["T"] < 3 and p["PLANE"] % 3 == 0,
    "pad_columns": lambda p: p["family"] == "private" and p["HWX"] > p["oh"] * p["ow"],
}


# ---- the operands --------------------------------------------------------------------------------------------------------
def route_of(case, n=None):
    """The case as a row of edge_cases.ROUTES (kind conv), at batch n."""
    s = case["shape"]
    return E._r(case["name"], "conv", ((s[0] if n is None else n),) + tuple(s[1:4]) + (s[4], s[5], s[5]) + tuple(s[6:]), impl=case["impl"])


def acts_of(case):
    """The conv's activations a case runs: EDGE_ACTS with the stated seeds, else one of edge_cases.ACTS by the case's place in
    the table.  [(act, alpha, seed)]."""
    if case["seeds"]:
        return [(a, al, s) for (a, al), s in zip(EDGE_ACTS, case["seeds"])]
    i = CASES.index(case)
    return [E.ACTS[i % len(E.ACTS)] + (6000 + i,)]


def add_tail(plref, c, seed):
    """dwconv_cases.add_tail's residual and calib copies, plus the tail without a calib copy (z alone)."""
    D.add_tail(plref, c, seed)
    c["tails"]["res_relu_f32"] = dict(c["tails"]["res_relu"], q=None, pre_q=None)
    return c


def make(plref, case, act, alpha, seed, n=None):
    """Operands and the oracle's results of one case (edge_cases.make_case's dict for kind conv, plus the tails)."""
    return add_tail(plref, E.make_case(plref, route_of(case, n), act, alpha, False, seed), seed)


def make_nondyadic(plref, case, act, alpha, seed=0):
    """The same shapes with scales that are no powers of two, biases and a residual off every grid, and calib scale 0.3: what
    the fp32 epilogue's fused multiply-add and the calib's multiply by 1 / scale round is then visible."""
    rng = np.random.default_rng([seed, 77, CASES.index(case)])
    n, cin, h, w, cout, k, pads, st, dl, g = case["shape"]
    s = E._plshape(plref, n, cin, h, w, cout, k, k, pads, st, dl, g)
    kk = (cin // g) * k * k
    es, ts = E.channel_plan(cout)
    x = E.activations(rng, (n, cin, h, w))
    wt = E.weights(rng, (cout, cin // g, k, k), kk, es, ts)
    acc = plref.conv2d_acc(s, x, wt)
    scale = (rng.uniform(0.55, 0.95, cout) * 2.0 ** -es).astype(np.float32)
    bias = rng.uniform(-40, 40, cout).astype(np.float32)
    pre = plref.epilogue(acc, scale, bias, act, alpha, False)
    res = rng.uniform(-70, 70, pre.shape).astype(np.float32)
    c = {"x": x, "w": wt, "acc": acc, "scale": scale, "bias": bias, "pre": pre, "res": res, "calib": ND_CALIB, "act": act,
         "alpha": alpha, "tails": {}}
    for key, (use_res, relu, calib) in TAILS.items():
        z = plref.elementwise_add(pre, res, relu) if use_res else pre
        c["tails"][key] = {"res": res if use_res else None, "relu": relu, "z": z}
    return c


def _freeze(c):
    for v in list(c.values()) + [a for t in c["tails"].values() for a in t.values()]:
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


@functools.lru_cache(maxsize=None)
def _reference_nd(plref, name, act, alpha):
    return _freeze(make_nondyadic(plref, BY_NAME[name], act, alpha))


def reference_nondyadic(plref, name, act, alpha):
    return _reference_nd(plref, name, act, alpha)


# ---- the edges -----------------------------------------------------------------------------------------------------------
def case_misses(c, act, alpha):
    """Every edge one made case lacks (dwconv_cases' thresholds), over the conv output and the three calib copies."""
    miss = ["conv:" + m for m in D.stage_misses(E.edge_stats(c["pre"], act, alpha), act, alpha)]
    for key in D.TAILS:
        miss += ["%s:%s" % (key, m) for m in D.calib_misses(c["tails"][key], key, act, alpha)]
    return miss


def find_seeds(plref, case, limit=400):
    """The first seed per activation of EDGE_ACTS at which the oracle's results of `case` lack no edge (how the table's seeds
    were chosen; None where `limit` seeds do not do)."""
    found = []
    for act, alpha in EDGE_ACTS:
        found.append(next((s for s in range(limit) if not case_misses(make(plref, case, act, alpha, s), act, alpha)), None))
    return tuple(found)
