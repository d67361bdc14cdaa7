"""Operands that put the int8 epilogues on their edges (used by test_gpu_edges.py and its CPU guard in test_edge_cases.py).

The folded per-channel scale is dyadic (2^-e), so acc * s is exact, and the folded bias is a multiple of 1/4.  The weights of
output channel c are drawn so that acc * 2^-e_c spreads over about +-T_c LSB, T_c in 150..600; e_c cycles through 1..5, so the
results sit on quarters (exact ties k + 0.5 of both signs) as well as on eighths / 32nds (where a round-to-nearest-even
truncation of the doubled value differs from round-toward-zero).  One output of every channel is pinned to an anchor value
(+-127.5, +-0.5, the relu6 bound) through the bias.  The maximum-magnitude operands are +-127 / -128 with weights of
matching sign: |acc| > 2^24 where K > 1040, where (float)acc itself rounds.

Every helper returns plain numpy arrays; the reference is always plref.conv2d_acc / plref.epilogue."""
import numpy as np

ACT_NONE, ACT_RELU, ACT_RELU6, ACT_LEAKY = 0, 1, 2, 4
SX = 73.6  # standard deviation of integers uniform in [-127, 127]
EXPS = (1, 2, 3, 5, 2, 4, 1)
TARGETS = (150, 300, 220, 600, 450, 180, 260)
# (act, alpha) pairs every route runs: relu6 with an integer bound, a half-integer one (2 alpha odd) and one above the
# int8 range (2 alpha > 254); leaky with alphas whose products of quarter values land on ties
ACTS = ((ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_RELU6, 60.0), (ACT_RELU6, 60.5), (ACT_RELU6, 200.5), (ACT_LEAKY, 0.25),
        (ACT_LEAKY, 0.375))


def channel_plan(cout, shift=0):
    """Per output channel: the scale exponent e_c and the spread T_c (LSB)."""
    e = np.array([EXPS[(c + shift) % len(EXPS)] for c in range(cout)])
    t = np.array([TARGETS[(c + 2 * shift) % len(TARGETS)] for c in range(cout)], np.float64)
    return e, t


def activations(rng, shape):
    return rng.integers(-127, 128, shape).astype(np.int8)


def weights(rng, shape, k, es, ts, sx=SX):
    """int8 weights [cout, ...]: channel c so that std(acc_c) * 2^-e_c ~ T_c / 2 for K = k products with std(x) = sx."""
    w = np.zeros(shape, np.int8)
    per = shape[1:]
    for c in range(shape[0]):
        sw = ts[c] * 2.0 ** es[c] / 2 / (np.sqrt(k) * max(sx, 1.0))
        if sw >= 0.82:
            wb = int(min(127, max(1, round(sw * np.sqrt(3)))))
            w[c] = rng.integers(-wb, wb + 1, per)
        else:  # sparse +-1
            w[c] = rng.choice(np.array([-1, 1], np.int8), per) * (rng.random(per) < max(sw * sw / 0.67, 0.02))
    return w


def anchors(act, alpha):
    if act == ACT_RELU6:
        return (alpha, 0.5, 127.5, alpha + 0.25, 2.5, alpha - 0.5)
    if act == ACT_LEAKY:  # negative pre-activation values whose product with alpha is a tie / past the bound
        return (127.5, -1.5 / alpha, 0.5, -127.5 / alpha, -0.5 / alpha * 3, -200.0 / alpha)
    return (127.5, -127.5, 0.5, -0.5, 5.5, -6.5)


def fold(rng, acc, es, act, alpha):
    """The folded scale 2^-e_c and a bias (multiple of 1/4) that puts one output of each channel on an anchor value."""
    cout = acc.shape[1]
    scale = (2.0 ** -es.astype(np.float64)).astype(np.float32)
    per_c = np.moveaxis(acc, 1, 0).reshape(cout, -1)
    anc = anchors(act, alpha)
    bias = np.empty(cout, np.float32)
    for c in range(cout):
        j = int(rng.integers(per_c.shape[1]))
        b = anc[(c + int(rng.integers(len(anc)))) % len(anc)] - float(per_c[c, j]) * float(scale[c])
        bias[c] = np.float32(np.round(b * 4) / 4)
    return scale, bias


def maxmag_operands(rng, x_shape, w_shape, groups=1, depthwise=False):
    """+-127 / -128 activations and weights of matching sign per input channel (and a per-output-channel sign), -128 sprinkled
    through both: every product has the same sign, |acc| ~ K * 127^2."""
    cin = x_shape[1]
    sgn = np.where(rng.random(cin) < 0.5, -1, 1)
    neg = rng.random(x_shape) < 0.5
    xm = np.where(neg, -128, -127)
    x = np.where(sgn[None, :, None, None] > 0, 127, xm).astype(np.int8)
    cout = w_shape[0]
    osg = np.where(np.arange(cout) % 3 == 1, -1, 1)
    cpg = w_shape[1]
    first = np.arange(cout) if depthwise else (np.arange(cout) // (cout // groups)) * cpg
    isg = np.stack([sgn[f:f + cpg] for f in first])
    want = np.broadcast_to((osg[:, None] * isg).reshape(cout, cpg, 1, 1), w_shape)
    wneg = np.where(rng.random(w_shape) < 0.5, -128, -127)
    w = np.where(want > 0, 127, wneg).astype(np.int8)
    return x, w


def fold_maxmag(rng, acc):
    """Dyadic scales that bring |acc| down to ~200 LSB, quarter biases."""
    cout = acc.shape[1]
    per_c = np.abs(np.moveaxis(acc, 1, 0).reshape(cout, -1).astype(np.float64)).max(axis=1)
    es = np.maximum(0, np.round(np.log2(np.maximum(per_c, 1) / 200.0))).astype(np.int64)
    scale = (2.0 ** -es.astype(np.float64)).astype(np.float32)
    bias = (np.round(rng.uniform(-40, 40, cout) * 4) / 4).astype(np.float32)
    return scale, bias


def edge_stats(y_f32, act, alpha):
    """What the pre-rounding values (the fp32 epilogue, activation included) of an int8 output hit."""
    f = np.asarray(y_f32, np.float64).ravel()
    frac = np.abs(f - np.trunc(f))
    tie = frac == 0.5
    return {"n": f.size, "tie_pos": int((tie & (f > 0)).sum()), "tie_neg": int((tie & (f < 0)).sum()),
            "sat_pos": int((f > 127.5).sum()), "sat_neg": int((f < -127.5).sum()),
            "at_127_5": int((f == 127.5).sum()), "at_m127_5": int((f == -127.5).sum()),
            "clip": int((f == alpha).sum()) if act == ACT_RELU6 else 0,
            # fractions in (0.25, 0.5): there truncating the doubled value and rounding it to nearest even differ
            "rtz": int(((frac > 0.25) & (frac < 0.5)).sum())}


# ---- the routes ----------------------------------------------------------------------------------------------------------
# kind: conv (plhip_conv2d_int8), dw (plhip_depthwise_conv_int8), calib (fp32-input stem), image (uint8-image stem), dwpw
# (plhip_dwpw_fused_int8), dwconv (fusion G), fc, tail (plhip_conv2d_int8_fused: residual add + calib copy).
# shape: n, cin, h, w, cout, kh, kw, pads (t, b, l, r), stride, dil, groups; mm_cin: the input channels of the
# maximum-magnitude case (K > 1040 where the route admits it).  knobs: forced through plhip_debug_set, reset to `reset`.
G1 = "conv1x1s1_gemm_int8_mfma32x32x32"


def _r(name, kind, shape, impl=None, knobs=(), mm_cin=None, m=None, kernel=None, seed_row=None):
    return {"name": name, "kind": kind, "shape": shape, "impl": impl, "knobs": dict(knobs), "mm_cin": mm_cin, "m": m,
            "kernel": kernel or name, "seed_row": seed_row}


def case_seed(i, route, j=0, maxmag=False):
    """The seed of case j of ROUTES[i]: from the row's index, or from the number the row states where few channels need a draw
    that puts an output on every anchor (test_edge_cases.py checks that it does)."""
    return 7000 * maxmag + 100 * (i if route["seed_row"] is None else route["seed_row"]) + j


ROUTES = [
    _r("gemm_nchw", "conv", (2, 96, 6, 6, 80, 1, 1, (0,) * 4, 1, 1, 1), G1, {"GEMM_VARIANT": 1}, 1088),
    _r("gemm_vperm_lds", "conv", (2, 96, 6, 6, 80, 1, 1, (0,) * 4, 1, 1, 1), G1, {"GEMM_VARIANT": 2}, 1088),
    _r("gemm_ring", "conv", (2, 160, 4, 5, 256, 1, 1, (0,) * 4, 1, 1, 1), G1, {"GEMM_VARIANT": 3, "GEMM_AREG": 0}, 1088),
    _r("gemm_ring_ma1", "conv", (2, 160, 4, 5, 200, 1, 1, (0,) * 4, 1, 1, 1), G1, {"GEMM_VARIANT": 3, "GEMM_MA": 1}, 1088),
    _r("gemm_areg", "conv", (2, 128, 4, 8, 256, 1, 1, (0,) * 4, 1, 1, 1), G1, {"GEMM_VARIANT": 3, "GEMM_AREG": 1}, 1024),
    _r("gemm_wide_n4", "conv", (2, 128, 4, 8, 256, 1, 1, (0,) * 4, 1, 1, 1), G1, {"WIDE_NTT": 4}, 1024),
    _r("gemm_wide_n7", "conv", (2, 128, 4, 8, 256, 1, 1, (0,) * 4, 1, 1, 1), G1, {"WIDE_NTT": 7}, 512),
    _r("gemm_wide_n8", "conv", (2, 128, 4, 8, 256, 1, 1, (0,) * 4, 1, 1, 1), G1, {"WIDE_NTT": 8}, 512),
    _r("implicit_gemm_tr", "conv", (2, 24, 9, 16, 128, 5, 5, (2,) * 4, 1, 1, 1), "conv_implicit_gemm_int8_mfma32x32x32", {}, 48,
       kernel="gemm_tr_2x2"),
    _r("patch_s1", "conv", (2, 64, 8, 14, 96, 3, 3, (1,) * 4, 1, 1, 1), "conv_patch_gemm_int8_mfma32x32x32", {}, 128),
    _r("patch_s2", "conv", (2, 64, 12, 14, 96, 3, 3, (1,) * 4, 2, 1, 1), "conv_patch_s2_gemm_int8_mfma32x32x32", {}, 128),
    _r("direct3x3s2_mfma", "conv", (2, 3, 16, 16, 40, 3, 3, (1,) * 4, 2, 1, 1), "conv_3x3s2_direct_int8_mfma32x32x32"),
    _r("direct3x3s2_dot4", "conv", (2, 4, 16, 16, 24, 3, 3, (1,) * 4, 2, 1, 1), "conv_3x3s2_direct_int8_dot4"),
    _r("subsample1x1s2", "conv", (2, 48, 10, 12, 64, 1, 1, (0,) * 4, 2, 1, 1), "conv_im2col_gemm_int8_mfma32x32x32", {}, 1088),
    _r("im2col_dilated", "conv", (2, 8, 11, 11, 40, 3, 3, (2,) * 4, 1, 2, 1), "conv_im2col_gemm_int8_mfma32x32x32", {}, 128),
    _r("stem7x7s2", "conv", (1, 3, 20, 32, 64, 7, 7, (3,) * 4, 2, 1, 1), "conv_7x7s2_direct_int8_mfma32x32x32"),
    _r("stem_f32_calib", "calib", (2, 3, 16, 16, 32, 3, 3, (1,) * 4, 2, 1, 1)),
    _r("stem_u8_image", "image", (2, 3, 16, 16, 32, 3, 3, (1,) * 4, 2, 1, 1)),
    # the direct strip kernel's rows name the whole instance of the int8 output (kernel_for: 32-bit outputs are never staged)
    _r("dw3x3s1_direct", "dw", (2, 24, 14, 14, 24, 3, 3, (1,) * 4, 1, 1, 24), kernel="dw_direct KS=3 S=1 RS=7 STAGE=1 FASTV=1"),
    _r("dw3x3s1_unstaged", "dw", (2, 24, 14, 14, 24, 3, 3, (1,) * 4, 1, 1, 24), knobs={"DW_STAGE": 0},
       kernel="dw_direct KS=3 S=1 RS=7 STAGE=0 FASTV=1"),
    _r("dw3x3s2_general_fetch", "dw", (2, 24, 14, 14, 24, 3, 3, (1,) * 4, 2, 1, 24), knobs={"DW_FASTV": 0},
       kernel="dw_direct KS=3 S=2 RS=7 STAGE=1 FASTV=0"),
    _r("dw5x5s1_direct", "dw", (2, 16, 14, 14, 16, 5, 5, (2,) * 4, 1, 1, 16), kernel="dw_direct KS=5 S=1 RS=7 STAGE=1 FASTV=1"),
    _r("dw5x5s2_band", "dw", (2, 16, 14, 14, 16, 5, 5, (2,) * 4, 2, 1, 16), knobs={"DW5_DIRECT": 0}, kernel="dw_band"),
    _r("dw3x3_dilated_generic", "dw", (2, 12, 13, 11, 12, 3, 3, (2,) * 4, 1, 2, 12), kernel="dw_generic"),
    _r("dwpw_14x14", "dwpw", (2, 128, 14, 14, 128, 3, 3, (1,) * 4, 1, 1, 128), m=256),
    _r("dwpw_14x14_mtw2", "dwpw", (1, 512, 14, 14, 512, 3, 3, (1,) * 4, 1, 1, 512), m=512),
    _r("dwpw_stream", "dwpw", (1, 256, 28, 28, 256, 3, 3, (1,) * 4, 1, 1, 256), m=256),
    _r("dwpw_stream_112", "dwpw", (1, 32, 112, 112, 32, 3, 3, (1,) * 4, 1, 1, 32), m=64, kernel="dwpw_stream"),
    _r("dwpw_stream_56", "dwpw", (1, 128, 56, 56, 128, 3, 3, (1,) * 4, 1, 1, 128), m=128, kernel="dwpw_stream"),
    _r("dwpw_stream_s2", "dwpw", (1, 128, 56, 56, 128, 3, 3, (1,) * 4, 2, 1, 128), m=256, kernel="dwpw_stream"),
    _r("dwpw_stream_s2_112", "dwpw", (1, 64, 112, 112, 64, 3, 3, (1,) * 4, 2, 1, 64), m=128, kernel="dwpw_stream"),
    _r("dwpw_stream_s2_28", "dwpw", (1, 256, 28, 28, 256, 3, 3, (1,) * 4, 2, 1, 256), m=512, kernel="dwpw_stream"),
    _r("dwpw_7x7", "dwpw", (1, 512, 14, 14, 512, 3, 3, (1,) * 4, 2, 1, 512), m=1024),
    _r("dwpw_7x7_s1", "dwpw", (1, 1024, 7, 7, 1024, 3, 3, (1,) * 4, 1, 1, 1024), m=1024, kernel="dwpw_7x7"),
    _r("dw_conv1x1_fusion_g", "dwconv", (2, 384, 14, 14, 384, 3, 3, (1,) * 4, 1, 1, 384), m=64, kernel="dw_conv1x1"),
    _r("fc_dot4", "fc", (6, 64, 1, 1, 40, 1, 1, (0,) * 4, 1, 1, 1), mm_cin=1088),
    _r("fc_mfma", "fc", (6, 64, 1, 1, 40, 1, 1, (0,) * 4, 1, 1, 1), knobs={"FC_MFMA": 1}, mm_cin=1088),
    _r("conv_tail_res_calib", "tail", (2, 64, 6, 6, 96, 1, 1, (0,) * 4, 1, 1, 1), G1),
    # (new rows go last: a case's seed is its row's index)
    # the direct depthwise kernel's other strip heights (the 14 x 14 rows above give RS = 7 only): strips of 8 rows, staged,
    # power-of-two quads per row / strips of 4 rows, three quads per row: the smallest planes at which those instances differ.
    # 8 channels give the anchors 8 draws: seeds at which every one of them is hit
    _r("dw3x3s1_rs8", "dw", (2, 8, 8, 8, 8, 3, 3, (1,) * 4, 1, 1, 8), kernel="dw_direct KS=3 S=1 RS=8 STAGE=1 FASTV=1", seed_row=42),
    _r("dw3x3s1_rs4", "dw", (2, 8, 4, 12, 8, 3, 3, (1,) * 4, 1, 1, 8), kernel="dw_direct KS=3 S=1 RS=4 STAGE=1 FASTV=1", seed_row=47),
    # fusion G off the square 14 x 14 plane (dwconv_cases.py has the whole launch plan): stride 2 without left / top padding,
    # a 130-wide row (two 128-column segments, the second ragged, rows staged byte by byte; 16 channels: a stated seed), a ragged
    # last M group with an M tail
    _r("dw_conv1x1_s2_pl0", "dwconv", (2, 32, 9, 12, 32, 3, 3, (0, 1, 0, 1), 2, 1, 32), m=24, kernel="dw_conv1x1"),
    _r("dw_conv1x1_wide130", "dwconv", (1, 16, 3, 130, 16, 3, 3, (1,) * 4, 1, 1, 16), m=16, kernel="dw_conv1x1", seed_row=55),
    _r("dw_conv1x1_ragged_m", "dwconv", (1, 32, 14, 14, 32, 3, 3, (1,) * 4, 1, 1, 32), m=264, kernel="dw_conv1x1"),
]


class Knobs:
    """The route's knobs forced through plhip_debug_set for a `with` block, then back at KNOB_DEFAULTS."""

    def __init__(self, lib, knobs):
        self.lib, self.knobs = lib, knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            assert self.lib.plhip_debug_set(k.encode(), int(v)) == 0, k

    def __exit__(self, *a):
        for k in self.knobs:
            self.lib.plhip_debug_set(k.encode(), KNOB_DEFAULTS[k])


GEMM_IMPLS = (G1, "conv_implicit_gemm_int8_mfma32x32x32")
OUT_KINDS = {"i32": 0, "f32": 1, "i8": 2}  # plhip_out_kind
DW_PLAN_KINDS = {"dw": 0, "dwpw": 1, "dwconv": 2}  # plhip_debug_dw_plan's kind


def kernel_of(capi, route, cin, out):
    """The kernel the route's launch reaches (the route table's `kernel`) under the knobs in force.  The GEMM, depthwise and
    fused depthwise routes ask the library for its own launch plan (capi.gemm_plan_text, capi.dw_plan_text: csrc/gemm_plan.h,
    csrc/dw_plan.h, the functions the launchers execute): the plan's name, and for the direct depthwise kernel its template
    parameters too."""
    n, _, h, w, cout, kh, kw, pads, st, dl, g = route["shape"]
    kind = route["kind"]
    if kind == "conv" and route["impl"] in GEMM_IMPLS:
        d = capi.conv_desc(n, cin, h, w, cout, kh, kw, pads, (st, st), (dl, dl), g)
        return capi.gemm_plan_text(d, OUT_KINDS[out]).split(" ")[0]
    if kind in DW_PLAN_KINDS:
        d = capi.conv_desc(n, cin, h, w, cin, kh, kw, pads, (st, st), (dl, dl), cin)
        t = capi.dw_plan_text(d, DW_PLAN_KINDS[kind], route["m"] or 0, OUT_KINDS[out]).split(" ")
        return " ".join(t[:6]) if t[0] == "dw_direct" else t[0]
    if kind == "fc":
        return "fc_mfma" if route["knobs"].get("FC_MFMA", 0) and cin % 32 == 0 else "fc_dot4"
    return route["name"]


def kernel_for(route, out):
    """The kernel the route's row names for output kind `out`: the row's `kernel`; the direct depthwise kernel stages int8
    output only, so its 32-bit outputs run the row's instance unstaged."""
    return route["kernel"] if out == "i8" else route["kernel"].replace("STAGE=1", "STAGE=0")


# the value each knob has when nobody set it (the launchers' defaults)
KNOB_DEFAULTS = {"GEMM_VARIANT": 0, "GEMM_AREG": 1, "GEMM_MA": 0, "WIDE_NTT": 0, "DW_STAGE": 1, "DW_FASTV": 1, "DW5_DIRECT": 1,
                 "FC_MFMA": 0, "GEMM_TR": 1, "TR_CFG": 3, "GEMM_WIDE": 1}
# the dw stage's activation of a fused pair, cycled against the pw stage's
DW_ACTS = ((ACT_RELU6, 60.5), (ACT_LEAKY, 0.375), (ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_RELU6, 200.5))


def acts_of(route):
    if route["kind"] == "fc":
        return ((ACT_NONE, 0.0), (ACT_RELU, 0.0))
    if route["kind"] == "tail":
        return ((ACT_NONE, 0.0), (ACT_RELU, 0.0), (ACT_LEAKY, 0.25))
    return ACTS


def _plshape(plref, n, cin, h, w, cout, kh, kw, pads, st, dl, g):
    return plref.shape(n, cin, h, w, cout, kh, kw, pads, (st, st), (dl, dl), g)


def image_to_tensor_ref(src, means, scales):
    """BGR / RGB uint8 [n, h, w, 3] -> fp32 NCHW: (x - mean[c]) * scale[c], two fp32 roundings (image2tensor.cc)."""
    y = np.empty((src.shape[0], 3) + src.shape[1:3], np.float32)
    for c in range(3):
        y[:, c] = (src[..., c].astype(np.float32) - np.float32(means[c])) * np.float32(scales[c])
    return y


# image stem: channel 0 lands on the calib's ties (x - 127.5 with calib scale 1), channel 1 on halves past +-127, channel 2 plain
IMG_MEANS, IMG_SCALES, IMG_CALIB = (127.5, 100.0, 64.0), (1.0, 2.0, 1.0), 1.0


def make_case(plref, route, act, alpha, maxmag, seed):
    """Inputs and the oracle's results of one (route, activation) case.  Returns a dict: the operands of the route's entry
    point, acc (int32 reference), scale / bias / alpha (folded), ref_i8 / ref_f32, and pre (the fp32 values the int8 output
    rounds: what the edges are measured on)."""
    rng = np.random.default_rng(seed)
    n, cin, h, w, cout, kh, kw, pads, st, dl, g = route["shape"]
    kind = route["kind"]
    if maxmag and route["mm_cin"]:
        cin = route["mm_cin"]
    c = {"act": act, "alpha": alpha}
    if kind in ("dwpw", "dwconv"):
        return _fused_case(plref, route, act, alpha, maxmag, rng, c)
    if kind == "fc":
        k = cin
        if maxmag:
            x4, w4 = maxmag_operands(rng, (n, k, 1, 1), (cout, k, 1, 1))
            x, wt = x4.reshape(n, k), w4.reshape(cout, k).T.copy()
        else:
            es, ts = channel_plan(cout)
            x = activations(rng, (n, k))
            wt = weights(rng, (cout, k), k, es, ts).T.copy()
        acc = plref.gemm_acc(x, wt)
        acc4 = acc.reshape(n, cout, 1, 1)
        sc, bi = fold_maxmag(rng, acc4) if maxmag else fold(rng, acc4, es, act, alpha)
        c.update(x=x, w=wt, acc=acc, scale=sc, bias=bi)
        c["pre"] = plref.epilogue(acc4, sc, bi, act, alpha, False).reshape(n, cout)
        c["ref_i8"] = plref.epilogue(acc4, sc, bi, act, alpha, True).reshape(n, cout)
        c["ref_f32"] = c["pre"]
        # with dyadic scales the reference's two fp32 forms of fc (one fused multiply-add; product then bias) agree
        c["ref_f32_two_roundings"] = plref.fc(x, wt, bi, sc, act == ACT_RELU, False, route=1)[0]
        return c
    s = _plshape(plref, n, cin, h, w, cout, kh, kw, pads, st, dl, g)
    k = (cin // g) * kh * kw
    w_shape = (cout, cin // g, kh, kw)
    es, ts = channel_plan(cout)
    if kind == "image":
        src = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
        src[..., 1] = rng.integers(30, 171, (n, h, w))
        c["src"] = src
        x = plref.calib_f32_to_i8(image_to_tensor_ref(src, IMG_MEANS, IMG_SCALES), IMG_CALIB)
        wt = weights(rng, w_shape, k, es, ts, float(x.std()))
    elif kind == "calib":
        cs = np.float32(1.0 / 64)
        q = rng.integers(-135, 136, (n, cin, h, w)).astype(np.float32)
        half = rng.random(q.shape) < 0.4
        xf = ((q + np.where(half, np.float32(0.5), np.float32(0.0))) * cs).astype(np.float32)
        c["xf"], c["calib"] = xf, float(cs)
        x = plref.calib_f32_to_i8(xf, float(cs))
        wt = weights(rng, w_shape, k, es, ts, float(x.std()))
    elif maxmag:
        x, wt = maxmag_operands(rng, (n, cin, h, w), w_shape, g, depthwise=kind == "dw")
    else:
        x = activations(rng, (n, cin, h, w))
        wt = weights(rng, w_shape, k, es, ts)
    acc = plref.conv2d_acc(s, x, wt)
    sc, bi = fold_maxmag(rng, acc) if maxmag else fold(rng, acc, es, act, alpha)
    c.update(x=x, w=wt, acc=acc, scale=sc, bias=bi, cin=cin)
    c["pre"] = plref.epilogue(acc, sc, bi, act, alpha, False)
    c["ref_i8"] = plref.epilogue(acc, sc, bi, act, alpha, True)
    c["ref_f32"] = c["pre"]
    if kind == "tail":
        # residual in quarters and a calib scale of 1/2: y + res lands on the calib's ties (z * 2 = k + 0.5) and past +-127
        res = (np.round(rng.uniform(-70, 70, c["pre"].shape) * 4) / 4).astype(np.float32)
        relu = act == ACT_RELU
        z = plref.elementwise_add(c["pre"], res, relu)
        c.update(res=res, res_relu=relu, calib=0.5, ref_q=plref.calib_f32_to_i8(z, 0.5), ref_z=z)
        c["pre_q"] = (z.astype(np.float64) * 2).astype(np.float32)
    return c


def _fused_case(plref, route, act, alpha, maxmag, rng, c):
    n, cin, h, w, cout, kh, kw, pads, st, dl, g = route["shape"]
    m = route["m"]
    dw_act, dw_alpha = DW_ACTS[(ACTS.index((act, alpha)) if (act, alpha) in ACTS else 0) % len(DW_ACTS)]
    sd = _plshape(plref, n, cin, h, w, cin, 3, 3, pads, st, 1, cin)
    oh, ow = plref.out_dims(sd)
    e1, t1 = channel_plan(cin, 1)
    if maxmag:
        x, wd = maxmag_operands(rng, (n, cin, h, w), (cin, 1, 3, 3), depthwise=True)
    else:
        x = activations(rng, (n, cin, h, w))
        wd = weights(rng, (cin, 1, 3, 3), 9, e1, t1)
    acc1 = plref.conv2d_acc(sd, x, wd)
    s1, b1 = fold_maxmag(rng, acc1) if maxmag else fold(rng, acc1, e1, dw_act, dw_alpha)
    mid = plref.epilogue(acc1, s1, b1, dw_act, dw_alpha, True)
    pre1 = plref.epilogue(acc1, s1, b1, dw_act, dw_alpha, False)
    sp = _plshape(plref, n, cin, oh, ow, m, 1, 1, (0,) * 4, 1, 1, 1)
    e2, t2 = channel_plan(m, 2)
    if maxmag:  # the dw stage saturates (+-127) under an activation that keeps the sign: pw weights of matching sign
        sgn = np.sign(mid.astype(np.int32).sum(axis=(0, 2, 3)))
        osg = np.where(np.arange(m) % 3 == 1, -1, 1)
        wp = np.where(osg[:, None] * sgn[None, :] >= 0, 127, np.where(rng.random((m, cin)) < 0.5, -128, -127))
        wp = wp.astype(np.int8).reshape(m, cin, 1, 1)
    else:
        wp = weights(rng, (m, cin, 1, 1), cin, e2, t2, max(float(mid.std()), 1.0))
    acc = plref.conv2d_acc(sp, mid, wp)
    s2, b2 = fold_maxmag(rng, acc) if maxmag else fold(rng, acc, e2, act, alpha)
    c.update(x=x, w_dw=wd, s1=s1, b1=b1, dw_act=dw_act, dw_alpha=dw_alpha, mid=mid, pre_mid=pre1, w=wp, acc=acc, scale=s2,
             bias=b2, cin=cin)
    c["pre"] = plref.epilogue(acc, s2, b2, act, alpha, False)
    c["ref_i8"] = plref.epilogue(acc, s2, b2, act, alpha, True)
    c["ref_f32"] = c["pre"]
    return c
