"""-m gpu: the YOLOv3 head entry points of the C ABI on the device (csrc/yolo_ops.hip).  plhip_yolo_box_f32 against yolo_oracle
under its derived comparison rule (8 units of 2^-23 of the operands; zeros, clipped coordinates and NaN / inf classes equal) at
the smallest maps where each path can go wrong, outputs prefilled with 0xFF bytes; plhip_yolo_head_f32 as BYTES against the
single-scale call per map -> plhip_concat_f32 twice -> plhip_transpose_f32 on the device; both inside one captured graph; the
refusals, which launch nothing."""
import ctypes as C

import numpy as np
import pytest

import yolo_oracle as Y

pytestmark = pytest.mark.gpu
F32 = np.float32
ANCHORS = {1: [10, 13], 3: [10, 13, 16, 30, 33, 23]}

# (h, w, misalign): 4x4 reaches the quad path of the head and one partial tile; 3x3 the scalar path; 2x6 is not square (the
# grid_size = h quirk); 13x13 has hw = 169, tiles of 64 with a tail of 41; 8x8 with the bases 4 bytes off 16: the alignment fallback
MAPS = [(4, 4, 0), (3, 3, 0), (2, 6, 0), (13, 13, 0), (8, 8, 1)]


def _same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not bad.any(), "%s: %d of %d elements differ" % (what, bad.sum(), bad.size)


@pytest.mark.parametrize("h,w,mis", MAPS)
def test_yolo_box_against_the_oracle(gpu_ctx, h, w, mis):
    seed = 6100 + 16 * h + w
    for an in (1, 3):
        for c in (1, 3, 80):
            for n in (1, 3):
                x = Y.random_map(seed + an + c + n, n, an, c, h, w)
                img = Y.random_img_size(seed, n)
                for clip, sxy, thresh in ((True, 1.0, 0.5), (False, 1.05, 0.5), (True, 1.05, 0.0), (False, 1.0, 1.5)):
                    what = "yolo_box %dx%d an %d c %d n %d clip %d scale %g thresh %g misalign %d" % (h, w, an, c, n, clip, sxy, thresh, mis)
                    wb, ws, pt = Y.yolo_box(x, img, ANCHORS[an], c, thresh, 32, clip, sxy, parts=True)
                    if thresh == 0.5:
                        assert 0 < pt["keep"].sum() < pt["keep"].size, what  # cells on both sides of the threshold
                    elif thresh == 1.5:
                        assert not pt["keep"].any() and not wb.any() and not ws.any(), what
                    else:
                        assert pt["keep"].all(), what
                    gb, gs = gpu_ctx.yolo_box(x, img, ANCHORS[an], c, thresh, 32, clip, sxy, misalign=mis)
                    worst = Y.check_against(gb, gs, wb, ws, pt, what)
                    print(what, "worst box %.2f score %.2f units of 2^-23" % worst)


def _special_map(an, c, h, w):
    """NaN, +inf, -inf and +-88.8 in each of the five entries, one cell each, in an otherwise random map"""
    x = Y.random_map(6200, 2, an, c, h, w, obj_bias=1.0).reshape(2, an, 5 + c, h * w)
    vals = [np.nan, np.inf, -np.inf, 88.8, -88.8]
    cell = 0
    for e in range(5):
        for v in vals:
            x[cell % 2, cell % an, e, cell % (h * w)] = F32(v)
            cell += 1
    x[1, 0, 5, 3] = F32(np.nan)  # and a class logit
    return x.reshape(2, an * (5 + c), h, w)


@pytest.mark.parametrize("clip", [True, False])
def test_yolo_box_special_values(gpu_ctx, clip):
    an, c, h, w = 3, 3, 5, 7
    x = _special_map(an, c, h, w)
    img = np.array([[416, 608], [333, 500]], np.int32)
    for thresh in (0.0, 0.3):
        wb, ws, pt = Y.yolo_box(x, img, ANCHORS[an], c, thresh, 32, clip, 1.05, parts=True)
        assert np.isnan(ws).any() and np.isnan(pt["conf"]).any()
        if not clip:
            assert np.isnan(wb).any() and np.isposinf(wb).any() and np.isneginf(wb).any()
        gb, gs = gpu_ctx.yolo_box(x, img, ANCHORS[an], c, thresh, 32, clip, 1.05)
        Y.check_against(gb, gs, wb, ws, pt, "special values clip %d thresh %g" % (clip, thresh))
        hb, hs = gpu_ctx.yolo_head([x], img, [ANCHORS[an]], c, thresh, [32], clip, 1.05)
        _same_bytes(hb, gb, "head boxes, special values")
        _same_bytes(hs, np.ascontiguousarray(gs.transpose(0, 2, 1)), "head scores, special values")


# (h, w) of the scales, finest last as a YOLOv3 head lists them; 3 anchors each
SCALE_SETS = {"misaligned": [(3, 3), (6, 6), (12, 12)], "quads": [(4, 4), (8, 8)], "one": [(4, 6)], "one_quad": [(8, 8)],
              "eight": [(1, 1), (2, 2), (2, 6), (4, 4), (3, 3), (8, 8), (5, 4), (2, 2)]}


@pytest.mark.parametrize("name", sorted(SCALE_SETS))
def test_yolo_head_equals_the_separate_ops(gpu_ctx, name):
    maps = SCALE_SETS[name]
    k = len(maps)
    anchors = [[10 + 3 * i, 13 + i, 16 + i, 30, 33, 23 + 2 * i] for i in range(k)]
    if name == "eight":
        anchors[2] = [10, 13]          # the scales need not share an anchor count
        anchors[5] = anchors[5] + [59, 119]
    ratios = [32 >> (i % 3) for i in range(k)]
    for n, c in ((1, 1), (3, 3), (2, 80)):
        xs = [Y.random_map(6300 + i, n, len(anchors[i]) // 2, c, h, w) for i, (h, w) in enumerate(maps)]
        img = Y.random_img_size(6301, n)
        for clip, sxy, thresh in ((True, 1.0, 0.5), (False, 1.05, 0.0)):
            what = "yolo_head %s n %d c %d clip %d" % (name, n, c, clip)
            single = [gpu_ctx.yolo_box(x, img, a, c, thresh, r, clip, sxy) for x, a, r in zip(xs, anchors, ratios)]
            want_b = gpu_ctx.concat([b for b, _s in single], 1)
            want_s = gpu_ctx.transpose(gpu_ctx.concat([s for _b, s in single], 1), (0, 2, 1))
            for mis in (0, 1):
                gb, gs = gpu_ctx.yolo_head(xs, img, anchors, c, thresh, ratios, clip, sxy, misalign=mis)
                _same_bytes(gb, want_b, what + " boxes misalign %d" % mis)
                _same_bytes(gs, want_s, what + " scores misalign %d" % mis)
            ob, os_, pt = Y.yolo_head(xs, img, anchors, c, thresh, ratios, clip, sxy, parts=True)
            Y.check_against(gb, gs, ob, os_, pt, what, score_layout="ncp")


def test_both_entry_points_in_one_captured_graph(gpu_ctx):
    L, h = gpu_ctx.L, gpu_ctx.h
    n, c, an = 2, 3, 3
    maps = [(4, 4), (3, 5)]
    anchors = [ANCHORS[3], [30, 61, 62, 45, 59, 119]]
    xs = [Y.random_map(6400 + i, n, an, c, hh, ww) for i, (hh, ww) in enumerate(maps)]
    img = Y.random_img_size(6401, n)
    want_box = gpu_ctx.yolo_box(xs[0], img, anchors[0], c, 0.5, 32, True, 1.0)
    want_head = gpu_ctx.yolo_head(xs, img, anchors, c, 0.5, [32, 16], True, 1.0)
    p0, p = an * 16, an * 16 + an * 15
    with gpu_ctx.scope() as s:
        dxs = [s.put(x) for x in xs]
        dimg = s.put(img)
        b_box, s_box, b_head, s_head = [s.out((cnt,), F32, fill=0xFF).ptr for cnt in (n * p0 * 4, n * p0 * c, n * p * 4, n * p * c)]
        gpu_ctx.sync()
        gpu_ctx.check(L.plhip_graph_begin(h), "graph_begin")
        st1 = gpu_ctx.yolo_box_launch(dxs[0], dimg, xs[0].shape, anchors[0], c, 0.5, 32, True, 1.0, b_box, s_box)
        st2 = gpu_ctx.yolo_head_launch(dxs, dimg, [x.shape for x in xs], anchors, c, 0.5, [32, 16], True, 1.0, b_head, s_head)
        graph = C.c_void_p()
        gpu_ctx.check(L.plhip_graph_end(h, C.byref(graph)), "graph_end")
        assert st1 == 0 and st2 == 0
        gpu_ctx.sync()
        # captured, not run: the outputs still hold the fill
        assert (gpu_ctx.to_host(b_box, (n * p0 * 4,), np.uint32) == 0xFFFFFFFF).all()
        gpu_ctx.check(L.plhip_graph_launch(h, graph), "graph_launch")
        gpu_ctx.sync()
        _same_bytes(gpu_ctx.to_host(b_box, (n, p0, 4), F32), want_box[0], "replayed yolo_box boxes")
        _same_bytes(gpu_ctx.to_host(s_box, (n, p0, c), F32), want_box[1], "replayed yolo_box scores")
        _same_bytes(gpu_ctx.to_host(b_head, (n, p, 4), F32), want_head[0], "replayed yolo_head boxes")
        _same_bytes(gpu_ctx.to_host(s_head, (n, c, p), F32), want_head[1], "replayed yolo_head scores")
        gpu_ctx.check(L.plhip_graph_destroy(h, graph), "graph_destroy")


def test_refusals_launch_nothing(gpu_ctx):
    L = gpu_ctx.L
    with gpu_ctx.scope() as s:
        x = s.put(np.zeros(3 * 8 * 16, F32))
        img = s.put(np.array([[100, 100]], np.int32))
        out = s.out((1024,), F32, fill=0xFF).ptr
        good = dict(x=x, img=img, shape=(1, 24, 4, 4), anchors=ANCHORS[3], c=3, ratio=32, boxes=out, scores=out)

        def box(**kw):
            a = dict(good, **kw)
            return gpu_ctx.yolo_box_launch(a["x"], a["img"], a["shape"], a["anchors"], a["c"], 0.5, a["ratio"], True, 1.0, a["boxes"], a["scores"])

        def head(count=1, **kw):
            a = dict(good, **kw)
            return gpu_ctx.yolo_head_launch([a["x"]] * count, a["img"], [a["shape"]] * count, [a["anchors"]] * count, a["c"], 0.5,
                                            [a["ratio"]] * count, True, 1.0, a["boxes"], a["scores"])

        def refused(f, status, part, **kw):
            st = f(**kw)
            msg = L.plhip_last_error(gpu_ctx.h).decode()
            assert st == status and msg.startswith("plhip_yolo_%s_f32: " % f.__name__) and part in msg, (f.__name__, kw, st, msg)

        for f in (box, head):
            refused(f, -1, "null x", x=None)
            refused(f, -1, "null img_size", img=None)
            refused(f, -1, "null boxes or scores", boxes=None)
            refused(f, -1, "null boxes or scores", scores=None)
            refused(f, -1, "n and c", shape=(0, 24, 4, 4))
            refused(f, -1, "n and c", c=0)
            refused(f, -1, "h and w", shape=(1, 24, 0, 4))
            refused(f, -1, "h and w", shape=(1, 24, 4, -1))
            refused(f, -1, "downsample_ratio", ratio=0)
            refused(f, -1, "anchor", anchors=[])
            refused(f, -3, "16 anchors", anchors=list(range(1, 35)))
            refused(f, -3, "2^31", shape=(1 << 20, 24, 32, 32))            # n * P alone
            refused(f, -3, "2^31", shape=(1, 24, 1 << 15, 1 << 15))        # P alone
            refused(f, -3, "2^31", shape=(2, 24, 1 << 12, 1 << 12), c=80)  # only with the classes: 2 * 3 * 2^24 * 80
            refused(f, -3, "downsample_ratio * h", shape=(1, 24, 1 << 12, 4), ratio=1 << 19)
        refused(head, -1, "anchor", anchors=[10, 13, 16])                  # an odd list
        refused(head, -1, "count", count=0)
        refused(head, -1, "count", count=9)
        refused(head, -3, "2^18", c=(1 << 18) + 1)
        assert L.plhip_yolo_box_f32(None, x, img, 1, 3, 3, 4, 4, (C.c_int * 6)(*ANCHORS[3]), 0.5, 32, 1, 1.0, out, out) == -1
        gpu_ctx.sync()
        assert (gpu_ctx.to_host(out, (1024,), np.uint32) == 0xFFFFFFFF).all()
        # and the accepted calls write: 48 boxes (4 floats each) in front of 48 x 3 scores
        scores = C.c_void_p(out.value + 4 * 192)
        assert box(scores=scores) == 0
        gpu_ctx.sync()
        first = gpu_ctx.to_host(out, (1024,), np.uint32)
        assert not (first[:336] == 0xFFFFFFFF).any() and (first[336:] == 0xFFFFFFFF).all()
        assert (first[192:336].view(F32) == F32(0.25)).all()               # sigmoid(0) = 0.5 is not below 0.5: conf * 0.5
        assert head(scores=scores) == 0
        gpu_ctx.sync()
        assert np.array_equal(gpu_ctx.to_host(out, (1024,), np.uint32), first)  # one class value everywhere: the layouts agree
