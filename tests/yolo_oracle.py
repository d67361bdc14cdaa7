"""yolo_box, stated once in numpy float32 with every operation rounded on its own (no test imports the device code from here), as
the reference computes it: lite/backends/arm/math/yolo_box.cc:24-178 behind lite/kernels/arm/yolo_box_compute.cc:25-51 and
lite/operators/yolo_box_op.cc:25-60.

X is [N, an * (5 + C), H, W]: entry e (x, y, w, h, objectness, C classes) of anchor a is channel a * (5 + C) + e (:49-57).
ImgSize is int32 [N, 2] = (height, width) of every image (:131-132).  What decides results, kept as written there:
  * sigmoid(v) = 1.f / (1.f + expf(-v)) (:24);
  * grid_size is H for BOTH x and y, and input_size = downsample_ratio * H (:113, :152-153): on a map that is not square the
    y centre is still divided by H and the anchor heights by ratio * H;
  * bias = -0.5 * (scale_x_y - 1.) is computed in double and narrowed (yolo_box_compute.cc:37);
  * a cell is skipped iff conf < conf_thresh (:139-142): a NaN objectness is kept and propagates into its scores;
  * skipped cells are the zeros of the memsets (:124-127) in Boxes [N, an * H * W, 4] and Scores [N, an * H * W, C];
  * the box of cell (row k, column l) of anchor a is box a * H * W + k * W + l (:160);
  * centre = (l + sigmoid(x0) * scale + bias) * img_w / grid, extent = exp(x2) * anchor_w * img_w / input_size, in this order of
    operations, every operand converted to float (:40-46); the corners are centre -+ extent / 2, a division (:65-68);
  * the clip is `v > 0 ? v : 0` for the near corner and `v < img - 1 ? v : img - 1` for the far one (:70-81): a NaN becomes 0
    and img - 1.
exp is evaluated in float64 and rounded once: a correctly rounded expf.  yolo_box_f64 is an independent evaluation of the same
formulas in float64 (no intermediate rounding), the cross-check of this file on the CPU.

The reference's own function could not be compiled on an x86 host to record goldens from: yolo_box.cc includes
lite/backends/arm/math/funcs.h, which includes <arm_neon.h>.  The oracle is pinned by the float64 evaluation
and by hand-computed cells.

The comparison rule (check_against) is derived, not chosen: two correct expf differ by at most 2 ulp; through 1 / (1 + e), the
affine map and the products that gives |got - want| <= 8 * 2^-23 * (|centre| + |half extent|) for a box coordinate (the bound
scales with the operands because centre - extent / 2 cancels) and 8 * 2^-23 * want for a non-zero score.  Which cells are zero,
the zeros, every coordinate the clip replaced and the class (NaN / +inf / -inf / finite) of every element must be equal.  No
objectness may lie within 32 * 2^-23 * conf_thresh of conf_thresh: assert_clear_of_threshold, asserted before a comparison."""
import numpy as np

import detection_oracle as D

F32 = np.float32
ULP = 2.0 ** -23


def exp32(v):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp(np.asarray(v, F32).astype(np.float64)).astype(F32)


def sigmoid(v):
    """yolo_box.cc:24"""
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(1) / (F32(1) + exp32(-np.asarray(v, F32)))


def bias_of(scale_x_y):
    """yolo_box_compute.cc:37: float scale_x_y widened, the product in double, narrowed"""
    return F32(-0.5 * (float(F32(scale_x_y)) - 1.0))


def check_dims(x_shape, img_shape, anchors, class_num):
    """YoloBoxOp::CheckShape (yolo_box_op.cc:40-45)"""
    anchors = list(anchors)
    if len(x_shape) != 4:
        raise ValueError("yolo_box: X must have rank 4, has %d" % len(x_shape))
    if not anchors or len(anchors) % 2:
        raise ValueError("yolo_box: anchors must hold (width, height) pairs, has %d values" % len(anchors))
    if class_num <= 0:
        raise ValueError("yolo_box: class_num must be positive")
    if x_shape[1] != (len(anchors) // 2) * (5 + class_num):
        raise ValueError("yolo_box: X has %d channels, anchors and class_num need %d" % (x_shape[1], (len(anchors) // 2) * (5 + class_num)))
    if len(img_shape) != 2 or img_shape[0] != x_shape[0] or img_shape[1] != 2:
        raise ValueError("yolo_box: ImgSize must be [%d, 2], is %r" % (x_shape[0], tuple(img_shape)))


def yolo_box(x, img_size, anchors, class_num, conf_thresh, downsample_ratio, clip_bbox=True, scale_x_y=1.0, parts=False):
    """Boxes [N, an * H * W, 4], Scores [N, an * H * W, C]; parts: also a dict of the intermediates the comparison rule needs, each
    [N, an * H * W(, 4)]: conf, keep, centre and half (per coordinate), replaced (the clip replaced the coordinate)."""
    x = np.asarray(x, F32)
    img_size = np.asarray(img_size, np.int32)
    check_dims(x.shape, img_size.shape, anchors, class_num)
    n, _ch, h, w = x.shape
    an = len(anchors) // 2
    e = x.reshape(n, an, 5 + class_num, h, w)
    scale, bias = F32(scale_x_y), bias_of(scale_x_y)
    grid, input_size = F32(h), F32(int(downsample_ratio) * h)
    img_h = img_size[:, 0].astype(F32).reshape(n, 1, 1, 1)
    img_w = img_size[:, 1].astype(F32).reshape(n, 1, 1, 1)
    col = np.arange(w, dtype=F32).reshape(1, 1, 1, w)
    row = np.arange(h, dtype=F32).reshape(1, 1, h, 1)
    aw = np.asarray(anchors[0::2], np.int32).astype(F32).reshape(1, an, 1, 1)
    ah = np.asarray(anchors[1::2], np.int32).astype(F32).reshape(1, an, 1, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        conf = sigmoid(e[:, :, 4])
        keep = ~(conf < F32(conf_thresh))                                        # :140
        cx = ((col + sigmoid(e[:, :, 0]) * scale) + bias) * img_w / grid         # :40
        cy = ((row + sigmoid(e[:, :, 1]) * scale) + bias) * img_h / grid         # :41-42
        bw = exp32(e[:, :, 2]) * aw * img_w / input_size                         # :43-44
        bh = exp32(e[:, :, 3]) * ah * img_h / input_size                         # :45-46
        hx, hy = bw / F32(2), bh / F32(2)
        raw = np.stack([cx - hx, cy - hy, cx + hx, cy + hy], axis=-1)            # :65-68
        boxes = raw.copy()
        replaced = np.zeros(raw.shape, bool)
        if clip_bbox:                                                            # :70-81
            lim = [None, None, np.broadcast_to(img_w - F32(1), cx.shape), np.broadcast_to(img_h - F32(1), cx.shape)]
            for k in (0, 1):
                ok = raw[..., k] > 0
                boxes[..., k] = np.where(ok, raw[..., k], F32(0))
                replaced[..., k] = ~ok
            for k in (2, 3):
                ok = raw[..., k] < lim[k]
                boxes[..., k] = np.where(ok, raw[..., k], lim[k])
                replaced[..., k] = ~ok
        scores = conf[:, :, None] * sigmoid(e[:, :, 5:])                         # :92, [N, an, C, H, W]
    boxes = np.where(keep[..., None], boxes, F32(0)).astype(F32).reshape(n, an * h * w, 4)
    scores = np.where(keep[:, :, None], scores, F32(0)).astype(F32).transpose(0, 1, 3, 4, 2).reshape(n, an * h * w, class_num)
    boxes, scores = np.ascontiguousarray(boxes), np.ascontiguousarray(scores)
    if not parts:
        return boxes, scores
    p = an * h * w
    centre = np.stack([np.broadcast_to(cx, keep.shape), np.broadcast_to(cy, keep.shape)] * 2, axis=-1).reshape(n, p, 4)
    half = np.stack([hx, hy] * 2, axis=-1).reshape(n, p, 4)
    return boxes, scores, {"conf": conf.reshape(n, p), "keep": keep.reshape(n, p), "centre": centre, "half": half,
                           "replaced": (replaced & keep[..., None]).reshape(n, p, 4), "conf_thresh": F32(conf_thresh)}


def yolo_box_f64(x, img_size, anchors, class_num, conf_thresh, downsample_ratio, clip_bbox=True, scale_x_y=1.0):
    """The same op cell by cell in float64 with no intermediate rounding (python floats and math.exp): written apart from
    yolo_box on purpose, loops instead of arrays.  Finite inputs only."""
    import math
    x = np.asarray(x, F32)
    n, _ch, h, w = x.shape
    an = len(anchors) // 2
    boxes = np.zeros((n, an * h * w, 4), np.float64)
    scores = np.zeros((n, an * h * w, class_num), np.float64)
    bias = float(bias_of(scale_x_y))
    scale = float(F32(scale_x_y))
    thresh = float(F32(conf_thresh))

    def sg(v):
        return 1.0 / (1.0 + math.exp(-float(v)))

    for i in range(n):
        ih, iw = int(img_size[i][0]), int(img_size[i][1])
        for a in range(an):
            ent = x[i, a * (5 + class_num):(a + 1) * (5 + class_num)]
            for k in range(h):
                for l in range(w):
                    conf = sg(ent[4, k, l])
                    if conf < thresh:
                        continue
                    cx = (l + sg(ent[0, k, l]) * scale + bias) * iw / h
                    cy = (k + sg(ent[1, k, l]) * scale + bias) * ih / h
                    bw = math.exp(float(ent[2, k, l])) * anchors[2 * a] * iw / (downsample_ratio * h)
                    bh = math.exp(float(ent[3, k, l])) * anchors[2 * a + 1] * ih / (downsample_ratio * h)
                    b = [cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]
                    if clip_bbox:
                        b = [b[0] if b[0] > 0 else 0.0, b[1] if b[1] > 0 else 0.0, b[2] if b[2] < iw - 1 else iw - 1.0,
                             b[3] if b[3] < ih - 1 else ih - 1.0]
                    idx = a * h * w + k * w + l
                    boxes[i, idx] = b
                    scores[i, idx] = [conf * sg(ent[5 + c, k, l]) for c in range(class_num)]
    return boxes, scores


def yolo_head(xs, img_size, anchors, class_num, conf_thresh, downsample_ratios, clip_bbox=True, scale_x_y=1.0, parts=False):
    """yolo_box per feature map -> concat(axis 1) of the Boxes and of the Scores -> transpose(0, 2, 1) of the Scores:
    boxes [N, P, 4], scores [N, C, P].  parts: the intermediates concatenated along P."""
    res = [yolo_box(x, img_size, a, class_num, conf_thresh, r, clip_bbox, scale_x_y, parts=True) for x, a, r in zip(xs, anchors, downsample_ratios)]
    boxes = np.concatenate([r[0] for r in res], axis=1)
    scores = D.transpose(np.concatenate([r[1] for r in res], axis=1), (0, 2, 1))
    if not parts:
        return boxes, scores
    pt = {k: (np.concatenate([r[2][k] for r in res], axis=1) if k != "conf_thresh" else res[0][2][k]) for k in res[0][2]}
    return boxes, scores, pt


# ------------------------------------------------------------------ the comparison rule
def assert_clear_of_threshold(pt, what=""):
    """No objectness within 32 * 2^-23 * conf_thresh of conf_thresh: the cells two correct implementations may disagree on."""
    t = float(pt["conf_thresh"])
    conf = pt["conf"].astype(np.float64)
    near = np.abs(conf - t) <= 32 * ULP * abs(t)
    near &= np.isfinite(conf) & (t != 0.0)   # at threshold 0 no finite sigmoid is below it: nothing is skipped either way
    assert not near.any(), "%s: %d objectness values within 32 ulp of conf_thresh %g: choose another seed" % (what, near.sum(), t)


def _classes(v):
    return np.where(np.isnan(v), 3, np.where(np.isposinf(v), 2, np.where(np.isneginf(v), 1, 0)))


def check_against(got_boxes, got_scores, want_boxes, want_scores, pt, what="", score_layout="npc"):
    """Asserts the rule of this file's head on device outputs; the scores in [N, P, C] ("npc") or [N, C, P] ("ncp").  Returns the
    worst box and score errors in units of 2^-23 * scale (bounds: 8)."""
    assert_clear_of_threshold(pt, what)
    assert got_boxes.shape == want_boxes.shape and got_boxes.dtype == F32, what
    assert got_scores.shape == want_scores.shape and got_scores.dtype == F32, what
    if score_layout == "ncp":
        got_scores, want_scores = got_scores.transpose(0, 2, 1), want_scores.transpose(0, 2, 1)
    keep = pt["keep"]
    # the skipped cells: all bits zero
    gb, gs = got_boxes.view(np.uint32), np.ascontiguousarray(got_scores).view(np.uint32)
    assert not gb[~keep].any(), "%s: a skipped cell's box is not all zero bits" % what
    assert not gs[~keep].any(), "%s: a skipped cell's scores are not all zero bits" % what
    # the class of every element
    assert np.array_equal(_classes(got_boxes), _classes(want_boxes)), "%s: NaN / inf / finite class of a box coordinate differs" % what
    assert np.array_equal(_classes(got_scores), _classes(want_scores)), "%s: NaN / inf / finite class of a score differs" % what
    # which elements are zero
    assert np.array_equal(got_scores == 0, want_scores == 0), "%s: the zero scores differ" % what
    # coordinates the clip replaced: exact
    rep = pt["replaced"]
    assert np.array_equal(got_boxes[rep].view(np.uint32), want_boxes[rep].view(np.uint32)), "%s: a clipped coordinate differs" % what
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(want_boxes) & keep[..., None] & ~rep
        unit = ULP * (np.abs(pt["centre"].astype(np.float64)) + np.abs(pt["half"].astype(np.float64)))
        err_b = np.abs(got_boxes.astype(np.float64) - want_boxes.astype(np.float64))
        worst_b = float((err_b[fin] / np.maximum(unit[fin], 1e-300)).max()) if fin.any() else 0.0
        bad = fin & (err_b > 8 * unit)
        assert not bad.any(), "%s: %d box coordinates beyond 8 * 2^-23 * (|centre| + |half extent|), worst %.2f units" % (what, bad.sum(), worst_b)
        fs = np.isfinite(want_scores) & (want_scores != 0)
        err_s = np.abs(got_scores.astype(np.float64) - want_scores.astype(np.float64))
        unit_s = ULP * np.abs(want_scores.astype(np.float64))
        worst_s = float((err_s[fs] / unit_s[fs]).max()) if fs.any() else 0.0
        bad = fs & (err_s > 8 * unit_s)
        assert not bad.any(), "%s: %d scores beyond 8 * 2^-23 * score, worst %.2f units" % (what, bad.sum(), worst_s)
    return worst_b, worst_s


# ------------------------------------------------------------------ seeded inputs
def random_map(seed, n, an, class_num, h, w, obj_bias=0.0, spread=1.5):
    """A head's feature map: logits of a trained head's range; obj_bias moves the objectness."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, an, 5 + class_num, h, w)) * spread).astype(F32)
    x[:, :, 4] += F32(obj_bias)
    return np.ascontiguousarray(x.reshape(n, an * (5 + class_num), h, w))


def random_img_size(seed, n):
    """A different (height, width) per image"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(200, 700, n), rng.integers(200, 700, n)], axis=1).astype(np.int32)


# ------------------------------------------------------------------ networks with a YOLOv3 head (workloads.yolov3_mini_net)
def ins_of(o):
    return [o["src"], o["img_size"]] if o["op"] == "yolo_box" else D.ins_of(o)


def outs_of(o):
    return list(o["names"]) if o["op"] == "yolo_box" else D.outs_of(o)


def plan(net):
    """detection_oracle.plan with yolo_box's two operands and two outputs; the int32 feed is no tensor to cast."""
    from shuffle_oracle import INT8_OPS
    ops = net["ops"]
    consumers = {}
    for i, o in enumerate(ops):
        for v in ins_of(o):
            consumers.setdefault(v, []).append(i)
    steps, prec, cast = [], {net["input"]: "f32", net["img_size"]: "i32"}, {}
    for o in ops:
        is8 = o["op"] in INT8_OPS
        want = "i8" if is8 else "f32"
        use = []
        for v in ins_of(o):
            if prec[v] != want and prec[v] != "i32":
                if v not in cast:
                    assert want == "i8", "int8 -> fp32 casts do not occur in these graphs"
                    cast[v] = v + "/precision_trans"
                    steps.append(("calib", dict(src=v, dst=cast[v], scale=float(o["in_scale"]))))
                use.append(cast[v])
            else:
                use.append(v)
        int8_out, oscale = False, 1.0
        if is8:
            cs = consumers.get(o["name"], [])
            int8_out = bool(cs) and all(ops[c]["op"] in INT8_OPS for c in cs) and o["name"] != net["output"]
            if int8_out:
                oscale = float(ops[cs[0]]["in_scale"])
        steps.append(("op", dict(o=o, ins=use, int8_out=int8_out, oscale=oscale)))
        for v in outs_of(o):
            prec[v] = "i8" if int8_out else "f32"
    return steps


def forward(plref, net, feeds):
    """name -> tensor for every variable of the unfused lowered program of a net with a YOLOv3 head; feeds: {"image": fp32 NCHW,
    "img_size": int32 [N, 2]}.  yolo_box is this file's; add and nearest_interp are plref's and interp_oracle's; every other op
    is one detection_oracle.forward knows and goes through _delegate.
    "<boxes>/parts" holds the intermediates of the comparison rule for every yolo_box."""
    import interp_oracle as I
    T = {net["input"]: np.ascontiguousarray(feeds[net["input"]], F32), net["img_size"]: np.ascontiguousarray(feeds[net["img_size"]], np.int32)}
    out = {}

    def put(name, val):
        T[name] = out[name] = val

    for kind, s in plan(net):
        if kind == "calib":
            put(s["dst"], plref.calib_f32_to_i8(T[s["src"]], s["scale"]))
            continue
        o, ins = s["o"], s["ins"]
        t = o["op"]
        if t == "yolo_box":
            b, sc, pt = yolo_box(T[ins[0]], T[ins[1]], o["anchors"], o["class_num"], o["conf_thresh"], o["downsample_ratio"], o["clip_bbox"],
                                 o["scale_x_y"], parts=True)
            put(o["names"][0], b)
            put(o["names"][1], sc)
            out[o["names"][0] + "/parts"] = pt
        elif t == "add":
            put(o["name"], plref.elementwise_add(T[ins[0]], T[ins[1]], o["act"] == "relu"))
        elif t == "nearest_interp":
            put(o["name"], I.interp(T[ins[0]], (o["out_h"], o["out_w"]), "nearest", o["align_corners"], o["align_mode"]))
        else:
            for k, v in _delegate(plref, s, T).items():
                put(k, v)
    return out


def _delegate(plref, s, T):
    """A step of an op detection_oracle.forward knows.  An op of one fp32 operand runs through that function itself, as a net of
    that op alone; a conv (whose kernel pick is this plan's), a concat and the NMS (several operands) through the functions it calls
    for them."""
    import shuffle_oracle as S
    o, ins = s["o"], s["ins"]
    t = o["op"]
    if t in ("conv2d", "depthwise_conv2d"):
        x = T[ins[0]]
        cout, _cg, k, _ = o["w"].shape
        p, d = o["pad"], o.get("dilation", 1)
        sh = plref.shape(x.shape[0], x.shape[1], x.shape[2], x.shape[3], cout, k, k, (p, p, p, p), (o["stride"],) * 2, (d, d), o["groups"])
        y, _ = plref.conv2d(sh, x, o["w"], o["bias"], float(o["in_scale"]), o["w_scale"], s["oscale"], o["act"], o["act_coef"], s["int8_out"])
        return {o["name"]: y}
    if t == "concat":
        return {o["name"]: S.concat([T[v] for v in ins], o["axis"])}
    if t == "multiclass_nms":
        return {o["name"] + k: v for k, v in D.nms_padded(T[ins[0]], T[ins[1]], o).items()}
    return D.forward(plref, dict(ops=[dict(o, src="in")], input="in", output=o["name"]), T[ins[0]])
