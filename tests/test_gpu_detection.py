"""-m gpu: the detection-head entry points of the C ABI on the device (csrc/transpose_ops.hip, csrc/detection_ops.hip) against
detection_oracle.  plhip_transpose_f32 as bytes over every permutation of ranks 2 to 4, the SSD shapes (tile edges, unaligned rows),
the quad path and a base off 16 bytes; plhip_concat_nhwc_f32 as bytes against transpose -> reshape -> concat; plhip_box_coder_decode_f32
within the project's fp32 rule (the device's expf is not numpy's); plhip_multiclass_nms_f32's out / count / index EQUAL to the
oracle's on the same inputs: the corner rules, random clustered boxes, both score layouts, both cuts on either side of their
counts, the largest envelope; the refusals, which launch nothing."""
import ctypes as C
import itertools

import numpy as np
import pytest

import detection_oracle as D

pytestmark = pytest.mark.gpu
F32 = np.float32


def _payload(rng, shape):
    """Distinct bit patterns (a counter), with NaNs of two payloads, infinities, -0.0 and denormals planted: a move keeps them all."""
    x = (np.arange(int(np.prod(shape)), dtype=np.uint32) * np.uint32(2654435761) >> np.uint32(3)).astype(np.uint32)
    edge = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x80000001], np.uint32)
    n = min(x.size, edge.size)
    x[rng.permutation(x.size)[:n]] = edge[:n]
    return x.view(F32).reshape(shape)


def _same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not bad.any(), "%s: %d of %d elements differ" % (what, bad.sum(), bad.size)


# ------------------------------------------------------------------ transpose
def test_transpose_every_permutation(gpu_ctx):
    rng = np.random.default_rng(610)
    for shape in ((2, 3, 5, 7), (3, 5, 7), (5, 7)):
        x = _payload(rng, shape)
        for perm in itertools.permutations(range(len(shape))):
            _same_bytes(gpu_ctx.transpose(x, perm), D.transpose(x, perm), "transpose %s %s" % (shape, perm))


# the SSD head moves (tile edges, rows of 361 and 65 floats, extents of 1), both tile kernels with more than one tile per side
# (72 x 68: quads; 130 x 67: elements), rows copied whole behind a permuted front, and one tile axis of a single element
SHAPES = [((2, 12, 19, 19), (0, 2, 3, 1)), ((2, 126, 1, 1), (0, 2, 3, 1)), ((1, 33, 1, 65), (0, 2, 3, 1)), ((2, 1917, 21), (0, 2, 1)),
          ((2, 8, 4, 16), (0, 2, 3, 1)), ((3, 72, 68), (0, 2, 1)), ((130, 67), (1, 0)), ((2, 3, 4, 8), (1, 0, 2, 3)),
          ((2, 4, 3, 64), (3, 1, 0, 2)), ((1, 1, 1, 1), (3, 2, 1, 0)), ((2, 1, 5, 1), (2, 3, 0, 1)), ((4, 1, 1, 6), (3, 1, 2, 0))]


@pytest.mark.parametrize("shape,perm", SHAPES)
def test_transpose_shapes_aligned_and_not(gpu_ctx, shape, perm):
    x = _payload(np.random.default_rng(611), shape)
    want = D.transpose(x, perm)
    for mis in (0, 1, 3):
        _same_bytes(gpu_ctx.transpose(x, perm, misalign=mis), want, "transpose %s %s misalign %d" % (shape, perm, mis))


def test_transpose_refusals(gpu_ctx):
    L = gpu_ctx.L
    with gpu_ctx.scope() as s:
        buf = s.alloc(64)

        def call(dims, perm, x=buf, y=buf, rank=None):
            st = L.plhip_transpose_f32(gpu_ctx.h, x, (C.c_int64 * len(dims))(*dims), (C.c_int * len(perm))(*perm), len(dims) if rank is None else rank, y)
            return st, L.plhip_last_error(gpu_ctx.h).decode()

        for args, status, part in ((((2, 2), (0, 0)), -1, "permutation"), (((2, 2), (0, 2)), -1, "permutation"), (((2, 0), (1, 0)), -1, "at least 1"),
                                   (((2, 2, 2, 2, 2), (0, 1, 2, 3, 4)), -3, "rank"), (((4,), (0,)), -3, "rank"),
                                   (((1 << 20, 1 << 20, 2), (0, 1, 2)), -3, "2^40")):
            st, msg = call(*args)
            assert st == status and msg.startswith("plhip_transpose_f32: ") and part in msg, (args, st, msg)
        assert call((2, 2), (1, 0), x=None)[0] == -1 and call((2, 2), (1, 0), y=None)[0] == -1


# ------------------------------------------------------------------ concat_nhwc
# (channels, h, w) of the operands; k divides every channel count
HEADS = [(3, [(12, 5, 7)]), (4, [(16, 4, 4), (24, 3, 3)]), (21, [(63, 19, 19), (126, 10, 10), (126, 5, 5), (126, 3, 3), (126, 2, 2), (126, 1, 1)]),
         (4, [(12, 19, 19), (24, 10, 10), (24, 5, 5), (24, 3, 3), (24, 2, 2), (24, 1, 1)]), (1, [(68, 9, 8), (4, 1, 4)]),
         (2, [(2, 1, 1)] * 9)]


@pytest.mark.parametrize("k,parts", HEADS)
def test_concat_nhwc_equals_transpose_reshape_concat(gpu_ctx, k, parts):
    rng = np.random.default_rng(612)
    for n in (1, 3):
        xs = [_payload(rng, (n, c, h, w)) for c, h, w in parts]
        want = D.concat_nhwc(xs, k)
        for mis in (0, 1):
            got = gpu_ctx.concat_nhwc(xs, misalign=mis).reshape(want.shape)
            _same_bytes(got, want, "concat_nhwc %s n %d misalign %d" % (parts, n, mis))
    if len(parts) <= 2:  # and the device's own three ops
        y = np.concatenate([gpu_ctx.transpose(x, (0, 2, 3, 1)).reshape(x.shape[0], -1, k) for x in xs], axis=1)
        _same_bytes(gpu_ctx.concat_nhwc(xs).reshape(y.shape), y, "concat_nhwc against the device's transpose")


def test_concat_nhwc_refusals(gpu_ctx):
    L = gpu_ctx.L
    with gpu_ctx.scope() as s:
        buf = s.alloc(64)
        one = (C.c_int64 * 1)(2)
        ptr = (C.c_void_p * 1)(buf)
        for args, part in (((ptr, one, one, 0, 1, buf), "count"), ((ptr, one, one, 1, 0, buf), "n must"), ((ptr, (C.c_int64 * 1)(0), one, 1, 1, buf), "extent"),
                           (((C.c_void_p * 1)(None), one, one, 1, 1, buf), "null input"), ((ptr, one, one, 1, 1, None), "null ctx")):
            assert L.plhip_concat_nhwc_f32(gpu_ctx.h, *args) == -1 and part in L.plhip_last_error(gpu_ctx.h).decode(), part


# ------------------------------------------------------------------ box_coder
@pytest.mark.parametrize("cols", [1, 63, 65, 1917])
def test_box_coder_decode(gpu_ctx, cols):
    rng = np.random.default_rng(613 + cols)
    rows = 3
    for axis in (0, 1):
        m = cols if axis == 0 else rows
        lo = rng.random((m, 2)).astype(F32)
        prior = np.concatenate([lo, lo + F32(0.05) + rng.random((m, 2)).astype(F32) * F32(0.3)], axis=1)
        pvar = (0.05 + 0.3 * rng.random((m, 4))).astype(F32)
        target = rng.standard_normal((rows, cols, 4)).astype(F32)
        for kw in ({"prior_var": pvar}, {"variance": [0.1, 0.1, 0.2, 0.2]}, {}):
            for normalized in (True, False):
                want = D.box_coder_decode(prior, target, axis=axis, normalized=normalized, **kw)
                for mis in (0, 1):
                    got = gpu_ctx.box_coder_decode(prior, target, axis=axis, normalized=normalized, misalign=mis, **kw)
                    what = "box_coder cols %d axis %d %s normalized %d misalign %d" % (cols, axis, sorted(kw), normalized, mis)
                    print(what, "max abs diff %.3g" % np.abs(got - want).max())
                    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5, err_msg=what)
                # without an exponent to evaluate (target w, h = 0: exp(0) == 1 on both sides) the arithmetic is fully specified
                t0 = target.copy()
                t0[..., 2:] = 0
                _same_bytes(gpu_ctx.box_coder_decode(prior, t0, axis=axis, normalized=normalized, **kw),
                            D.box_coder_decode(prior, t0, axis=axis, normalized=normalized, **kw), "box_coder centres")


def test_box_coder_refusals(gpu_ctx):
    L = gpu_ctx.L
    with gpu_ctx.scope() as s:
        buf = s.alloc(64)
        for args, part in (((buf, None, None, buf, 0, 1, 0, 1, buf), "at least 1"), ((buf, None, None, buf, 1, 1, 2, 1, buf), "axis"),
                           ((None, None, None, buf, 1, 1, 0, 1, buf), "null ctx"), ((buf, None, None, buf, 1, 1, 0, 1, None), "null ctx")):
            assert L.plhip_box_coder_decode_f32(gpu_ctx.h, *args) == -1 and part in L.plhip_last_error(gpu_ctx.h).decode(), part


# ------------------------------------------------------------------ multiclass_nms
def _device_equals_oracle(ctx, pkg, boxes, scores, params, want, what, layouts=("ncp", "npc"), misalign=(0,)):
    n, c, p = scores.shape
    rows, offsets, index = want[:3]
    wo, wc, wi = D.padded(rows, offsets, index, params["keep_top_k"])
    for layout in layouts:
        d = pkg.capi.nms_desc(n, c, p, layout=layout, **params)
        s = scores if layout == "ncp" else np.ascontiguousarray(scores.transpose(0, 2, 1))
        for mis in misalign:
            for with_index in (True, False):
                out, count, idx = ctx.multiclass_nms(boxes, s, d, with_index=with_index, misalign=mis)
                tag = "%s %s misalign %d index %d" % (what, layout, mis, with_index)
                assert count.tolist() == wc.tolist(), tag
                _same_bytes(out, wo, tag)
                if with_index:
                    assert np.array_equal(idx, wi), tag
                else:
                    assert idx is None


@pytest.mark.parametrize("name", sorted(D.corner_cases()))
def test_nms_corner_rule(gpu_ctx, pkg, name):
    boxes, scores, params, expected = D.corner_cases()[name]
    want = D.multiclass_nms(boxes, scores, **params)
    assert want[2].tolist() == expected
    _device_equals_oracle(gpu_ctx, pkg, boxes, scores, params, want, name, misalign=(0, 1))


@pytest.mark.parametrize("shape", D.RANDOM_SHAPES)
def test_nms_random_clustered_boxes(gpu_ctx, pkg, shape):
    for variant in ({}, {"background_label": -1, "nms_top_k": 20, "keep_top_k": 7}, {"normalized": False, "nms_threshold": 0.3}):
        boxes, scores, params, want = D.random_case(shape, **variant)
        if shape[2] > 1:  # some candidates are suppressed and some survive
            assert sum(s["suppressed"] for s in want[3]) > 0 and want[1][-1] > 0
        _device_equals_oracle(gpu_ctx, pkg, boxes, scores, params, want, "nms %s %s" % (shape, variant),
                              misalign=(0, 1) if shape[2] < 1000 else (0,))


def test_nms_cuts_on_either_side_of_their_counts(gpu_ctx, pkg):
    """nms_top_k below, at and above the largest candidate count of a class; keep_top_k below, at and above an image's total."""
    boxes, scores, params, want = D.random_case((2, 3, 65))
    most = int((scores[:, 1:] > F32(params["score_threshold"])).sum(axis=2).max())
    assert most > 4
    for top_k in (most - 1, most, most + 1, 1, -1):
        prm = dict(params, nms_top_k=top_k)
        _device_equals_oracle(gpu_ctx, pkg, boxes, scores, prm, D.multiclass_nms(boxes, scores, **prm), "nms_top_k %d of %d" % (top_k, most))
    totals = [s["kept"] for s in want[3]]
    assert min(totals) > 2
    for keep in sorted({min(totals) - 1, min(totals), max(totals), max(totals) + 1, 1}):
        prm = dict(params, keep_top_k=keep)
        res = D.multiclass_nms(boxes, scores, **prm)
        assert np.diff(res[1]).tolist() == [min(t, keep) for t in totals]
        _device_equals_oracle(gpu_ctx, pkg, boxes, scores, prm, res, "keep_top_k %d of %s" % (keep, totals))


def test_nms_largest_envelope(gpu_ctx, pkg):
    """P = 16384 with nms_top_k = keep_top_k = 4096: the largest LDS block stage A may ask for (148 KB), more than 4096 candidates
    in a class so that the cut at nms_top_k falls inside the sorted keys; and 4 classes x 4096 = 16384 list slots in stage B."""
    n, c, p = 1, 5, 16384
    rng = np.random.default_rng(614)
    boxes = D.clustered_case(614, n, 1, p)[0]
    scores = (rng.random((n, c, p)) * 0.04).astype(F32)
    scores[0, 1, rng.permutation(p)[:4500]] = (0.05 + rng.random(4500)).astype(F32)   # 4500 candidates, cut at 4096
    scores[0, 2, rng.permutation(p)[:300]] = (0.05 + rng.random(300)).astype(F32)
    scores[0, 4, :] = F32(0.5)                                                          # 16384 equal scores: prior order
    boxes[0, :, :] += (np.arange(p, dtype=F32) * F32(0.25))[:, None]                   # thin the clusters: most boxes survive
    params = dict(background_label=0, score_threshold=0.05, nms_top_k=4096, nms_threshold=0.45, keep_top_k=4096, normalized=True)
    want = D.multiclass_nms(boxes, scores, return_stats=True, **params)
    assert want[3][0]["kept"] > 4096 and want[3][0]["suppressed"] > 0 and want[3][0]["empty_classes"] == 1
    _device_equals_oracle(gpu_ctx, pkg, boxes, scores, params, want, "largest envelope", layouts=("ncp",))


def test_nms_refusals_launch_nothing(gpu_ctx, pkg):
    capi, L = pkg.capi, gpu_ctx.L
    with gpu_ctx.scope() as sc:
        boxes = sc.put(np.zeros((1, 8, 4), F32))
        scores = sc.put(np.ones((1, 2, 8), F32))
        ws = sc.alloc(4096)
        sentinel = np.full(64, 7.0, F32)
        out = sc.put(sentinel)
        count = sc.put(np.full(4, 7, np.int32))
        good = dict(background_label=0, score_threshold=0.01, nms_top_k=4, nms_threshold=0.45, keep_top_k=4)

        def call(d, b=boxes, s=scores, w=ws, o=out, c=count):
            st = L.plhip_multiclass_nms_f32(gpu_ctx.h, b, s, C.byref(d) if d is not None else None, w, o, None, c)
            return st, L.plhip_last_error(gpu_ctx.h).decode()

        for d, status, part in ((capi.nms_desc(1, 2, 8, **dict(good, nms_eta=0.9)), -3, "nms_eta"), (capi.nms_desc(1, 2, 8, **dict(good, keep_top_k=-1)), -1, "keep_top_k"),
                                (capi.nms_desc(1, 2, 16385, **good), -3, "16384 priors"), (capi.nms_desc(1, 2, 5000, **dict(good, nms_top_k=-1)), -3, "4096"),
                                (capi.nms_desc(1, 9000, 8, **dict(good, nms_top_k=-1, keep_top_k=8)), -3, "above 16384"), (capi.nms_desc(0, 2, 8, **good), -1, "at least 1")):
            st, msg = call(d)
            assert st == status and msg.startswith("plhip_multiclass_nms_f32: ") and part in msg, (st, msg)
        ok = capi.nms_desc(1, 2, 8, **good)
        assert call(None)[0] == -1 and call(ok, b=None)[0] == -1 and call(ok, s=None)[0] == -1 and call(ok, w=None)[0] == -1
        assert call(ok, w=C.c_void_p(ws.value + 4))[0] == -1 and call(ok, o=None)[0] == -1 and call(ok, c=None)[0] == -1
        gpu_ctx.sync()
        assert np.array_equal(gpu_ctx.to_host(out, (64,), F32), sentinel) and gpu_ctx.to_host(count, (4,), np.int32).tolist() == [7] * 4
        assert call(ok)[0] == 0  # and the accepted call writes: one box of eight coincident ones survives
        assert gpu_ctx.to_host(count, (1,), np.int32).tolist() == [1]
