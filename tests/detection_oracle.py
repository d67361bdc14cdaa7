"""The detection-head ops, stated once in numpy float32 with every operation rounded on its own (no test imports the device code
from here): transpose, reshape, box_coder (decode_center_size) and multiclass_nms in the 3-D score form, as the reference computes
them (lite/kernels/arm/transpose_compute.cc, lite/operators/reshape_op.cc, lite/kernels/arm/box_coder_compute.cc:92-158,
lite/kernels/host/multiclass_nms_compute.cc:31-322).

The points of multiclass_nms that decide results:
  * a candidate needs score > score_threshold, so a NaN score never is one;
  * candidates are ordered by a STABLE sort on `first > second`: equal scores keep ascending prior index, -0.0 equals +0.0;
  * the list is cut at nms_top_k (negative: all);
  * a candidate is kept iff overlap <= nms_threshold against every box kept before it; the overlap is 0 for disjoint boxes, an
    inverted box has area 0, normalized == False adds 1 to every extent, and the value is inter / (a1 + a2 - inter): two coincident
    zero-area boxes give 0 / 0 = NaN, `NaN <= t` is false and the later box is suppressed;
  * the background label is skipped (-1: none);
  * where an image's total exceeds keep_top_k, a stable descending sort runs over the concatenation in (label ascending, order of
    selection), is cut at keep_top_k and regrouped by label in sorted order;
  * rows are (label, score, x1, y1, x2, y2); the index of a row is image * P + prior."""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------ transpose / reshape
def transpose(x, perm):
    x = np.asarray(x)
    perm = tuple(int(p) for p in perm)
    if not 2 <= x.ndim <= 4 or sorted(perm) != list(range(x.ndim)):
        raise ValueError("transpose: perm %r is not a permutation of rank %d (2 .. 4)" % (perm, x.ndim))
    return np.ascontiguousarray(np.transpose(x, perm))


def reshape_dims(in_dims, shape):
    """reshape_op.cc's ValidateShape for the `shape` attribute: 0 copies the input's dim at that place, one -1 is inferred."""
    in_dims = [int(d) for d in in_dims]
    shape = [int(s) for s in shape]
    if sum(s == -1 for s in shape) > 1:
        raise ValueError("reshape: more than one -1 in %r" % (shape,))
    out = []
    for i, s in enumerate(shape):
        if s == 0:
            if i >= len(in_dims):
                raise ValueError("reshape: 0 at place %d of %r beyond the input's rank" % (i, shape))
            out.append(in_dims[i])
        elif s == -1 or s > 0:
            out.append(s)
        else:
            raise ValueError("reshape: bad dim %d in %r" % (s, shape))
    total = int(np.prod(in_dims, dtype=np.int64))
    if -1 in out:
        rest = int(np.prod([d for d in out if d != -1], dtype=np.int64))
        if rest == 0 or total % rest != 0:
            raise ValueError("reshape: %r does not divide %r" % (shape, in_dims))
        out[out.index(-1)] = total // rest
    if int(np.prod(out, dtype=np.int64)) != total:
        raise ValueError("reshape: %r holds another count than %r" % (shape, in_dims))
    return out


def reshape(x, shape):
    x = np.ascontiguousarray(x)
    return x.reshape(reshape_dims(x.shape, shape))


def concat_nhwc(xs, k):
    """transpose(0,2,3,1) -> reshape([0,-1,k]) -> concat(axis 1) of NCHW tensors: the join of an SSD head."""
    return np.concatenate([reshape(transpose(x, (0, 2, 3, 1)), [0, -1, k]) for x in xs], axis=1)


# ------------------------------------------------------------------ prior_box
def expand_aspect_ratios(aspect_ratios, flip):
    """ExpandAspectRatios: 1 first, then every ratio not within 1e-6 (a float comparison) of one already there, with its reciprocal
    behind it when flip."""
    out = [F32(1)]
    for ar in aspect_ratios:
        ar = F32(ar)
        if any(abs(F32(ar - o)) < F32(1e-6) for o in out):
            continue
        out.append(ar)
        if flip:
            out.append(F32(1) / ar)
    return out


def prior_box(feat_hw, img_hw, min_sizes, max_sizes=(), aspect_ratios=(), variances=(0.1, 0.1, 0.2, 0.2), flip=True, clip=False,
              step_w=0.0, step_h=0.0, offset=0.5, min_max_aspect_ratios_order=False):
    """(Boxes, Variances), each [H, W, A, 4] float32, in the reference's order of operations: min_size and max_size are truncated to
    int; step = float(image) / feature where a step is 0; centre = (index + offset) * step; a box is ((cx - w / 2) / image_w, (cy - h /
    2) / image_h, (cx + w / 2) / image_w, (cy + h / 2) / image_h); per min_size: the square of min_size, then (unless
    min_max_aspect_ratios_order puts it second) the ratios other than 1 with w = min_size * sqrt(ar), h = min_size / sqrt(ar), then
    the square of sqrt(min_size * max_size)."""
    h, w = (int(v) for v in feat_hw)
    img_h, img_w = (int(v) for v in img_hw)
    step_w, step_h = F32(step_w), F32(step_h)
    if step_w == 0 or step_h == 0:
        step_w = F32(img_w) / F32(w)
        step_h = F32(img_h) / F32(h)
    if max_sizes and len(max_sizes) != len(min_sizes):
        raise ValueError("prior_box: one max_size per min_size, or none")
    cx = ((np.arange(w, dtype=F32) + F32(offset)) * step_w)[None, :]
    cy = ((np.arange(h, dtype=F32) + F32(offset)) * step_h)[:, None]
    ars = expand_aspect_ratios(aspect_ratios, flip)
    two = F32(2)

    def box(bw, bh):
        bw, bh = F32(bw), F32(bh)
        x0 = np.broadcast_to((cx - bw / two) / F32(img_w), (h, w))
        y0 = np.broadcast_to((cy - bh / two) / F32(img_h), (h, w))
        x1 = np.broadcast_to((cx + bw / two) / F32(img_w), (h, w))
        y1 = np.broadcast_to((cy + bh / two) / F32(img_h), (h, w))
        return np.stack([x0, y0, x1, y1], axis=-1)

    priors = []
    for s, mn in enumerate(min_sizes):
        mn = int(F32(mn))
        first = [box(mn, mn)]
        big = [box(np.sqrt(F32(mn * int(F32(max_sizes[s])))), np.sqrt(F32(mn * int(F32(max_sizes[s])))))] if max_sizes else []
        com = [box(F32(mn) * np.sqrt(ar), F32(mn) / np.sqrt(ar)) for ar in ars if not abs(float(ar) - 1.0) < 1e-6]
        priors += first + (big + com if min_max_aspect_ratios_order else com + big)
    boxes = np.stack(priors, axis=2).astype(F32)
    if clip:
        boxes = np.minimum(np.maximum(boxes, F32(0)), F32(1))
    var = np.broadcast_to(np.asarray(variances, F32), boxes.shape).copy()
    return np.ascontiguousarray(boxes), var


# ------------------------------------------------------------------ box_coder, decode_center_size
def box_coder_decode(prior, target, prior_var=None, variance=None, axis=0, normalized=True, dtype=F32):
    """target [rows, cols, 4]; the prior box (and its variance in prior_var) of element (i, j) is row j with axis 0, row i with
    axis 1.  Variance: prior_var if given, else the four values of `variance` if given, else none.  dtype float64 evaluates the
    same formulas in double (the cross-check of test_detection_host.py)."""
    t = np.asarray(target, dtype)
    p = np.asarray(prior, dtype)
    if t.ndim != 3 or t.shape[2] != 4 or p.ndim != 2 or p.shape[1] != 4:
        raise ValueError("box_coder: target [rows, cols, 4] and prior [., 4] expected")
    if axis not in (0, 1) or p.shape[0] != t.shape[1 - axis]:
        raise ValueError("box_coder: prior rows %d do not match axis %d of %r" % (p.shape[0], axis, t.shape))
    bc = (lambda a: a[None, :]) if axis == 0 else (lambda a: a[:, None])
    nn = dtype(0 if normalized else 1)
    two = dtype(2)
    if prior_var is not None:
        v = np.asarray(prior_var, dtype)
        if v.shape != p.shape:
            raise ValueError("box_coder: prior_var %r differs from prior %r" % (v.shape, p.shape))
        var = [bc(v[:, k]) for k in range(4)]
    elif variance is not None and len(variance):
        var = [dtype(F32(variance[k])) for k in range(4)]
    else:
        var = [dtype(1)] * 4
    pw = bc(p[:, 2] - p[:, 0] + nn)
    ph = bc(p[:, 3] - p[:, 1] + nn)
    pcx = bc(p[:, 0]) + pw / two
    pcy = bc(p[:, 1]) + ph / two
    cx = var[0] * t[..., 0] * pw + pcx
    cy = var[1] * t[..., 1] * ph + pcy
    w = np.exp(var[2] * t[..., 2]) * pw
    h = np.exp(var[3] * t[..., 3]) * ph
    out = np.stack([cx - w / two, cy - h / two, cx + w / two - nn, cy + h / two - nn], axis=-1)
    assert out.dtype == dtype
    return out


# ------------------------------------------------------------------ multiclass_nms
def bbox_area(b, normalized):
    """b [..., 4] float32 -> area, 0 for an inverted box."""
    w = b[..., 2] - b[..., 0]
    h = b[..., 3] - b[..., 1]
    area = w * h if normalized else (w + F32(1)) * (h + F32(1))
    return np.where((b[..., 2] < b[..., 0]) | (b[..., 3] < b[..., 1]), F32(0), area).astype(F32)


def jaccard_overlap(b1, b2, normalized):
    """JaccardOverlap(box1, box2) broadcast over leading axes, float32, each operation rounded on its own."""
    b1 = np.asarray(b1, F32)
    b2 = np.asarray(b2, F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        disjoint = (b2[..., 0] > b1[..., 2]) | (b2[..., 2] < b1[..., 0]) | (b2[..., 1] > b1[..., 3]) | (b2[..., 3] < b1[..., 1])
        # std::max(a, b) is a < b ? b : a, std::min(a, b) is b < a ? b : a
        ixmin = np.where(b1[..., 0] < b2[..., 0], b2[..., 0], b1[..., 0])
        iymin = np.where(b1[..., 1] < b2[..., 1], b2[..., 1], b1[..., 1])
        ixmax = np.where(b2[..., 2] < b1[..., 2], b2[..., 2], b1[..., 2])
        iymax = np.where(b2[..., 3] < b1[..., 3], b2[..., 3], b1[..., 3])
        norm = F32(0 if normalized else 1)
        iw = ixmax - ixmin + norm
        ih = iymax - iymin + norm
        inter = iw * ih
        a1 = bbox_area(b1, normalized)
        a2 = bbox_area(b2, normalized)
        ov = inter / (a1 + a2 - inter)
    return np.where(disjoint, F32(0), ov).astype(F32)


def sorted_candidates(scores, score_threshold, top_k):
    """GetMaxScoreIndex: the priors with score > threshold, by a stable sort on descending score, cut at top_k (negative: all)."""
    scores = np.asarray(scores, F32)
    with np.errstate(invalid="ignore"):
        cand = [int(i) for i in np.nonzero(scores > F32(score_threshold))[0]]
    cand.sort(key=lambda i: -float(scores[i]))  # stable; -0.0 and +0.0 compare equal
    if top_k > -1 and top_k < len(cand):
        cand = cand[:top_k]
    return cand


def nms_fast(boxes, scores, score_threshold, nms_threshold, top_k, normalized):
    """NMSFast with eta >= 1: the kept priors in the order they were selected, and how many candidates were suppressed."""
    boxes = np.asarray(boxes, F32)
    kept = []
    suppressed = 0
    thr = F32(nms_threshold)
    for idx in sorted_candidates(scores, score_threshold, top_k):
        keep = True
        if kept:
            ov = jaccard_overlap(boxes[idx][None, :], boxes[kept], normalized)
            with np.errstate(invalid="ignore"):
                ok = ov <= thr
            keep = bool(ok.all())
        if keep:
            kept.append(idx)
        else:
            suppressed += 1
    return kept, suppressed


def multiclass_nms_image(boxes, scores, background_label, score_threshold, nms_top_k, nms_threshold, keep_top_k, normalized=True,
                         nms_eta=1.0):
    """One image: boxes [P, 4], scores [C, P].  Returns (label -> kept priors in output order, stats), stats = the number of kept
    boxes before the keep_top_k cut, the number of candidates suppressed by overlap, and the classes without a candidate."""
    if nms_eta < 1:
        raise ValueError("multiclass_nms: nms_eta < 1 (adaptive threshold) is not stated here")
    scores = np.asarray(scores, F32)
    indices = {}
    stats = {"kept": 0, "suppressed": 0, "empty_classes": 0}
    for c in range(scores.shape[0]):
        if c == background_label:
            continue
        indices[c], sup = nms_fast(boxes, scores[c], score_threshold, nms_threshold, nms_top_k, normalized)
        stats["suppressed"] += sup
        with np.errstate(invalid="ignore"):
            stats["empty_classes"] += int(not (scores[c] > F32(score_threshold)).any())
    stats["kept"] = sum(len(v) for v in indices.values())
    if keep_top_k > -1 and stats["kept"] > keep_top_k:
        pairs = [(float(scores[label][idx]), label, idx) for label in sorted(indices) for idx in indices[label]]
        pairs.sort(key=lambda t: -t[0])  # stable
        pairs = pairs[:keep_top_k]
        regrouped = {}
        for _s, label, idx in pairs:
            regrouped.setdefault(label, []).append(idx)
        indices = regrouped
    return {label: indices[label] for label in sorted(indices) if indices[label]}, stats


def multiclass_nms(boxes, scores, background_label, score_threshold, nms_top_k, nms_threshold, keep_top_k, normalized=True,
                   nms_eta=1.0, return_stats=False):
    """boxes [N, P, 4], scores [N, C, P] -> the reference's LoD form: (rows [M, 6], offsets [N + 1], index [M]) with
    rows = (label, score, x1, y1, x2, y2) and index = image * P + prior.  The "no detection at all" case ([[-1]] and offsets
    [0, 1]) is `detections_lod`'s business; here M is 0 then."""
    boxes = np.asarray(boxes, F32)
    scores = np.asarray(scores, F32)
    n, p = boxes.shape[:2]
    if boxes.ndim != 3 or boxes.shape[2] != 4 or scores.ndim != 3 or scores.shape[0] != n or scores.shape[2] != p:
        raise ValueError("multiclass_nms: boxes [N, P, 4] and scores [N, C, P] expected, got %r and %r" % (boxes.shape, scores.shape))
    rows, index, offsets, all_stats = [], [], [0], []
    for i in range(n):
        sel, stats = multiclass_nms_image(boxes[i], scores[i], background_label, score_threshold, nms_top_k, nms_threshold,
                                          keep_top_k, normalized, nms_eta)
        all_stats.append(stats)
        for label, idxs in sel.items():
            for idx in idxs:
                rows.append(np.concatenate([np.array([label, scores[i, label, idx]], F32), boxes[i, idx]]))
                index.append(i * p + idx)
        offsets.append(len(rows))
    out = (np.stack(rows).astype(F32) if rows else np.zeros((0, 6), F32), np.array(offsets, np.int64), np.array(index, np.int32))
    return out + (all_stats,) if return_stats else out


def padded(rows, offsets, index, keep_top_k):
    """The device's fixed-size form of `multiclass_nms`'s result: out [N, keep_top_k, 6] and index [N, keep_top_k] filled with -1
    past an image's count, and count [N]."""
    n = len(offsets) - 1
    out = np.full((n, keep_top_k, 6), -1, F32)
    idx = np.full((n, keep_top_k), -1, np.int32)
    count = np.zeros(n, np.int32)
    for i in range(n):
        s, e = int(offsets[i]), int(offsets[i + 1])
        count[i] = e - s
        out[i, :e - s] = rows[s:e]
        idx[i, :e - s] = index[s:e]
    return out, count, idx


def detections_lod(out, count, index=None):
    """The reference's output form from the padded one: (rows [M, 6], batch offsets, index [M, 1] or None).  No detection in any
    image: rows [[-1]] with offsets [0, 1] without an index output, rows [0, 6] and index [0, 1] with one
    (multiclass_nms_compute.cc:361-370)."""
    out = np.asarray(out, F32)
    count = np.asarray(count).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    if offsets[-1] == 0:
        if index is None:
            return np.array([[-1]], F32), np.array([0, 1], np.int64), None
        return np.zeros((0, 6), F32), offsets, np.zeros((0, 1), np.int32)
    rows = np.concatenate([out[i, :count[i]] for i in range(len(count))], axis=0)
    idx = None if index is None else np.concatenate([np.asarray(index)[i, :count[i]] for i in range(len(count))])[:, None].astype(np.int32)
    return rows, offsets, idx


# ------------------------------------------------------------------ a second, independent evaluation of NMS
def multiclass_nms_matrix(boxes, scores, background_label, score_threshold, nms_top_k, nms_threshold, keep_top_k, normalized=True):
    """Same result by another route: per class the full IoU matrix of the sorted candidates, then a greedy scan over a boolean
    `removed` mask (a kept box removes every later one it overlaps); the keep_top_k cut by one lexicographic sort on (score
    descending, label, position)."""
    boxes = np.asarray(boxes, F32)
    scores = np.asarray(scores, F32)
    n, p = boxes.shape[:2]
    rows, index, offsets = [], [], [0]
    for i in range(n):
        entries = []  # (label, position, prior)
        for c in range(scores.shape[1]):
            if c == background_label:
                continue
            s = scores[i, c]
            with np.errstate(invalid="ignore"):
                cand = np.nonzero(s > F32(score_threshold))[0]
            key = np.where(s[cand] == 0, F32(0), s[cand])  # -0.0 onto +0.0
            cand = cand[np.lexsort((cand, -key.astype(np.float64)))]
            if nms_top_k > -1:
                cand = cand[:nms_top_k]
            b = boxes[i, cand]
            iou = jaccard_overlap(b[:, None, :], b[None, :, :], normalized) if len(cand) else np.zeros((0, 0), F32)
            with np.errstate(invalid="ignore"):
                hit = ~(iou <= F32(nms_threshold))
            removed = np.zeros(len(cand), bool)
            pos = 0
            for k in range(len(cand)):
                if removed[k]:
                    continue
                entries.append((c, pos, int(cand[k])))
                pos += 1
                removed[k + 1:] |= hit[k + 1:, k]
        if len(entries) > keep_top_k > -1:
            sc = np.array([scores[i, c, pr] for c, _pos, pr in entries], np.float64)
            order = np.lexsort(([e[1] for e in entries], [e[0] for e in entries], -sc))[:keep_top_k]
            entries = sorted(entries[k] for k in order)
        for c, _pos, pr in entries:
            rows.append(np.concatenate([np.array([c, scores[i, c, pr]], F32), boxes[i, pr]]))
            index.append(i * p + pr)
        offsets.append(len(rows))
    return (np.stack(rows).astype(F32) if rows else np.zeros((0, 6), F32), np.array(offsets, np.int64), np.array(index, np.int32))


# ------------------------------------------------------------------ inputs the tests share
def clustered_case(seed, n, c, p, pass_share=0.3, inverted=0):
    """Random boxes in clusters (so that overlaps above and below any threshold occur) and scores of which about `pass_share`
    exceed 0.05, a few of them exactly equal inside a class and across classes.  boxes [N, P, 4], scores [N, C, P]."""
    rng = np.random.default_rng(seed)
    centres = rng.random((n, max(1, p // 6), 2)).astype(F32)
    which = rng.integers(0, centres.shape[1], (n, p))
    ctr = np.take_along_axis(centres, which[..., None].repeat(2, -1), axis=1) + (rng.standard_normal((n, p, 2)) * 0.02).astype(F32)
    half = (0.05 + 0.1 * rng.random((n, p, 2))).astype(F32)
    boxes = np.concatenate([ctr - half, ctr + half], axis=-1).astype(F32)
    for k in range(inverted):
        boxes[k % n, (7 * k + 1) % p, [0, 2]] = boxes[k % n, (7 * k + 1) % p, [2, 0]]
    scores = rng.random((n, c, p)).astype(F32)
    scores = np.where(scores < pass_share, F32(0.05) + scores, F32(0.04) * scores).astype(F32)
    if p >= 8:
        scores[:, :, p // 2] = scores[:, :, 1]                    # equal inside a class
        scores[:, 1:, 3] = scores[:, :1, 3].repeat(c - 1, axis=1)  # equal across classes
    return boxes, scores


def _disjoint_boxes(p):
    """p unit boxes two apart: no pair overlaps."""
    x = np.arange(p, dtype=F32) * F32(2)
    return np.stack([x, np.zeros(p, F32), x + F32(0.5), np.full(p, 0.5, F32)], axis=1)


def corner_cases():
    """name -> (boxes [N, P, 4], scores [N, C, P], params, expected index list): the rules above as literal small cases.  params
    are multiclass_nms's keyword arguments; expected is the index column (image * P + prior) the rules give by hand."""
    nan = F32(np.nan)
    base = dict(background_label=-1, score_threshold=0.01, nms_top_k=-1, nms_threshold=0.5, keep_top_k=8, normalized=True)
    cases = {}

    def add(name, boxes, scores, expected, **over):
        boxes = np.asarray(boxes, F32)
        scores = np.asarray(scores, F32)
        boxes = boxes[None] if boxes.ndim == 2 else boxes
        scores = scores[None] if scores.ndim == 2 else scores
        cases[name] = (boxes, scores, dict(base, **over), list(expected))

    # 2 / (4 + 2 - 2) == 0.5 exactly: overlap <= threshold keeps the second box
    add("iou_equal_to_threshold_is_kept", [[0, 0, 2, 2], [0, 0, 2, 1]], [[0.9, 0.8]], [0, 1])
    add("iou_just_above_threshold_is_suppressed", [[0, 0, 2, 2], [0, 0, 2, 1.001]], [[0.9, 0.8]], [0])
    # 0 / (0 + 0 - 0) is NaN, and NaN <= t is false
    add("coincident_zero_area_boxes", [[1, 1, 1, 1], [1, 1, 1, 1], [5, 5, 6, 6]], [[0.9, 0.8, 0.7]], [0, 2])
    # the inverted candidate is not "disjoint": inter = (-2)(-2) = 4, areas 0 and 4, 4 / 0 = inf
    add("inverted_box", [[0, 0, 2, 2], [2, 2, 0, 0], [7, 7, 6, 6]], [[0.9, 0.8, 0.7]], [0, 2])
    # touching boxes: inter 0 normalized; (0 + 1)(0 + 1) = 1 of areas 4 and 4 otherwise: 1 / 7 > 0.1
    add("touching_normalized", [[0, 0, 1, 1], [1, 1, 2, 2]], [[0.9, 0.8]], [0, 1], nms_threshold=0.1)
    add("touching_not_normalized", [[0, 0, 1, 1], [1, 1, 2, 2]], [[0.9, 0.8]], [0], nms_threshold=0.1, normalized=False)
    # equal scores: ascending prior inside a class, ascending label across classes; the cut keeps class 1 alone
    eq = np.full((3, 4), 0.5, F32)
    add("equal_scores_keep_top_k", _disjoint_boxes(4), eq, [0, 1, 2], background_label=0, keep_top_k=3)
    add("equal_scores_all_kept", _disjoint_boxes(4), eq, [0, 1, 2, 3, 0, 1, 2, 3], background_label=0, keep_top_k=8)
    add("equal_scores_top_k_inside_a_class", _disjoint_boxes(4), eq, [0, 1, 0, 1], background_label=0, nms_top_k=2)
    # -0.0 and +0.0 are equal: prior order, whatever the sign bit
    add("signed_zero_scores", _disjoint_boxes(4), [[-0.0, 0.0, -0.0, 0.0]], [0, 1, 2], score_threshold=-1.0, nms_top_k=3)
    add("nan_score_is_no_candidate", _disjoint_boxes(3), [[nan, 0.5, nan]], [1])
    add("nan_score_below_a_negative_threshold", _disjoint_boxes(3), [[nan, 0.5, -0.5]], [1, 2], score_threshold=-1.0)
    add("nms_top_k_all", _disjoint_boxes(6), [[0.1, 0.6, 0.2, 0.5, 0.3, 0.4]], [1, 3, 5, 4, 2, 0])
    add("nms_top_k_zero", _disjoint_boxes(3), [[0.1, 0.6, 0.2]], [], nms_top_k=0)
    two = np.array([[0.9, 0.1, 0.2], [0.3, 0.8, 0.005]], F32)
    add("background_none", _disjoint_boxes(3), two, [0, 2, 1, 1, 0], background_label=-1)
    add("background_one", _disjoint_boxes(3), two, [0, 2, 1], background_label=1)
    add("background_beyond_the_classes", _disjoint_boxes(3), two, [0, 2, 1, 1, 0], background_label=7)
    # image 1 of 2 has no score above the threshold
    bb = np.stack([_disjoint_boxes(3), _disjoint_boxes(3)])
    add("no_detection_in_one_image", bb, [[[0.001, 0.002, 0.003]], [[0.2, 0.9, 0.5]]], [4, 5, 3])
    add("no_detection_in_any_image", bb, np.zeros((2, 2, 3), F32), [])
    return cases


_RANDOM = {}
# (N, C, P) -> the variants run on it: (background, nms_top_k, keep_top_k)
RANDOM_SHAPES = [(1, 2, 1), (2, 3, 65), (3, 5, 300), (2, 21, 1917)]


def random_case(shape, background_label=0, nms_top_k=400, keep_top_k=200, nms_threshold=0.45, normalized=True):
    """(boxes, scores, params, (rows, offsets, index, stats)) of the clustered case of `shape`, computed once per argument set."""
    key = (shape, background_label, nms_top_k, keep_top_k, nms_threshold, normalized)
    if key not in _RANDOM:
        n, c, p = shape
        boxes, scores = clustered_case(590 + n + 3 * c + 7 * p, n, c, p, inverted=2 if p > 8 else 0)
        params = dict(background_label=background_label, score_threshold=0.05, nms_top_k=nms_top_k, nms_threshold=nms_threshold,
                      keep_top_k=keep_top_k, normalized=normalized)
        _RANDOM[key] = (boxes, scores, params, multiclass_nms(boxes, scores, return_stats=True, **params))
    return _RANDOM[key]


# ------------------------------------------------------------------ networks with detection heads (workloads.ssd_mini_net)
def ins_of(o):
    import shuffle_oracle as S
    t = o["op"]
    if t == "prior_box":
        return [o["src"], o["image"]]
    if t == "box_coder":
        return [o["prior"]] + ([o["prior_var"]] if o["prior_var"] else []) + [o["target"]]
    if t == "multiclass_nms":
        return [o["boxes"], o["scores"]]
    return S.ins_of(o)


def outs_of(o):
    if o["op"] == "prior_box":
        return list(o["names"])
    if o["op"] == "multiclass_nms":
        return [o["name"], o["name"] + "/count"] + ([o["index"]] if o["index"] else [])
    return [o["name"]]


def plan(net):
    """shuffle_oracle.plan for op lists with several operands or outputs per op: [(kind, dict)] in execution order, kind in
    {calib, op}.  The kernel pick is the reference's: an int8 op writes int8 iff every reader of its output is an int8 op."""
    from shuffle_oracle import INT8_OPS
    ops = net["ops"]
    consumers = {}
    for i, o in enumerate(ops):
        for v in ins_of(o):
            consumers.setdefault(v, []).append(i)
    steps, prec, cast = [], {net["input"]: "f32"}, {}
    for o in ops:
        is8 = o["op"] in INT8_OPS
        want = "i8" if is8 else "f32"
        use = []
        for v in ins_of(o):
            if prec[v] != want:
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


def forward(plref, net, image):
    """name -> tensor for every variable of the unfused lowered program of a detection net ("<var>/precision_trans" for calib
    outputs; a multiclass_nms output in the device's padded form, with "<name>/count"), and "<name>/stats" for the health checks."""
    import shuffle_oracle as S
    T = {net["input"]: np.ascontiguousarray(image, F32)}
    out = {}

    def put(name, val):
        T[name] = out[name] = val

    for kind, s in plan(net):
        if kind == "calib":
            put(s["dst"], plref.calib_f32_to_i8(T[s["src"]], s["scale"]))
            continue
        o, ins = s["o"], s["ins"]
        t = o["op"]
        if t in ("conv2d", "depthwise_conv2d"):
            x = T[ins[0]]
            cout, _cg, k, _ = o["w"].shape
            p, d = o["pad"], o.get("dilation", 1)
            sh = plref.shape(x.shape[0], x.shape[1], x.shape[2], x.shape[3], cout, k, k, (p, p, p, p), (o["stride"],) * 2, (d, d), o["groups"])
            y, _ = plref.conv2d(sh, x, o["w"], o["bias"], float(o["in_scale"]), o["w_scale"], s["oscale"], o["act"], o["act_coef"], s["int8_out"])
            put(o["name"], y)
        elif t == "concat":
            put(o["name"], S.concat([T[v] for v in ins], o["axis"]))
        elif t == "softmax":
            put(o["name"], plref.softmax(T[ins[0]]))
        elif t == "transpose":
            put(o["name"], transpose(T[ins[0]], o["perm"]))
        elif t == "reshape":
            put(o["name"], reshape(T[ins[0]], o["shape"]))
        elif t == "prior_box":
            b, v = prior_box(T[ins[0]].shape[2:], T[ins[1]].shape[2:], o["min_sizes"], o["max_sizes"], o["aspect_ratios"], o["variances"],
                             o["flip"], o["clip"], o["step_w"], o["step_h"], o["offset"], o["min_max_aspect_ratios_order"])
            put(o["names"][0], b)
            put(o["names"][1], v)
        elif t == "box_coder":
            put(o["name"], box_coder_decode(T[ins[0]], T[ins[-1]], prior_var=T[ins[1]] if len(ins) == 3 else None, variance=o["variance"],
                                            axis=o["axis"], normalized=o["normalized"]))
        elif t == "multiclass_nms":
            for k_, v_ in nms_padded(T[ins[0]], T[ins[1]], o).items():
                put(o["name"] + k_, v_)
        else:
            raise ValueError(t)
    return out


def nms_params(o):
    return dict(background_label=o["background_label"], score_threshold=o["score_threshold"], nms_top_k=o["nms_top_k"],
                nms_threshold=o["nms_threshold"], keep_top_k=o["keep_top_k"], normalized=o["normalized"], nms_eta=o["nms_eta"])


def nms_padded(boxes, scores, o):
    """{"": out, "/count": count, "/index": index, "/stats": per-image stats} of the multiclass_nms op dict `o` on boxes [N, P, 4] and
    scores [N, C, P]."""
    rows, offsets, index, stats = multiclass_nms(boxes, scores, return_stats=True, **nms_params(o))
    po, pc, pi = padded(rows, offsets, index, o["keep_top_k"])
    return {"": po, "/count": pc, "/index": pi, "/stats": stats}
