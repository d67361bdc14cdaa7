"""CPU tests of the detection-head ops: detection_oracle's multiclass_nms against a second, independent evaluation (full IoU matrix,
greedy scan over a boolean mask) and, where torchvision is installed, against torchvision.ops.nms; its box_coder against a float64
evaluation; the corner rules of the reference's host NMS as literal small cases; the reference's LoD output form from the padded
device form; reshape's shape rule; the exported symbols and their refusals; the kept ISA of csrc/detection_ops.hip (no private
segment, no fused multiply-add of the kernels' own arithmetic)."""
import ctypes as C
import glob
import itertools
import os
import re

import numpy as np
import pytest

import detection_oracle as D

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITE = os.path.join(ROOT, "paddle-lite_amd")
NEW_SYMBOLS = ("plhip_transpose_f32", "plhip_concat_nhwc_f32", "plhip_box_coder_decode_f32", "plhip_multiclass_nms_f32")


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) and np.asarray(x).shape == np.asarray(y).shape
               for x, y in zip(a, b))


# ------------------------------------------------------------------ the oracle against other evaluations
@pytest.mark.parametrize("shape", D.RANDOM_SHAPES)
def test_nms_oracle_equals_the_matrix_evaluation(shape):
    """Also what the GPU test relies on: in every random case some candidates are suppressed and some survive (P = 1 apart)."""
    for variant in ({}, {"background_label": -1, "nms_top_k": 20, "keep_top_k": 7}, {"normalized": False, "nms_threshold": 0.3}):
        boxes, scores, params, (rows, offsets, index, stats) = D.random_case(shape, **variant)
        other = D.multiclass_nms_matrix(boxes, scores, **params)
        assert _same((rows, offsets, index), other), (shape, variant)
        assert rows.shape == (offsets[-1], 6) and index.shape == (offsets[-1],)
        assert (np.diff(offsets) <= params["keep_top_k"]).all()
        if shape[2] > 1:
            assert sum(s["suppressed"] for s in stats) > 0 and offsets[-1] > 0, (shape, variant, stats)


def test_nms_oracle_random_cases_exercise_both_cuts():
    """The largest case has more candidates than nms_top_k in a class and more kept boxes than keep_top_k in an image."""
    boxes, scores, params, (_rows, offsets, _index, stats) = D.random_case((2, 21, 1917))
    assert (scores[:, 1:] > F32(params["score_threshold"])).sum(axis=2).max() > params["nms_top_k"]
    assert max(s["kept"] for s in stats) > params["keep_top_k"] and (np.diff(offsets) == params["keep_top_k"]).any()


def test_nms_oracle_equals_torchvision_for_one_class():
    tv = pytest.importorskip("torchvision")
    torch = pytest.importorskip("torch")
    boxes, scores = D.clustered_case(601, 1, 1, 300)
    rows, _off, index = D.multiclass_nms(boxes, scores, -1, 0.05, -1, 0.45, 300)
    cand = np.nonzero(scores[0, 0] > F32(0.05))[0]
    keep = tv.ops.nms(torch.from_numpy(boxes[0, cand]), torch.from_numpy(scores[0, 0, cand]), 0.45).numpy()
    # torchvision suppresses at iou > t on its own evaluation of the overlap: the sets agree unless an overlap sits within an ulp of t
    assert sorted(cand[keep].tolist()) == sorted(index.tolist())
    assert len(rows) == len(keep)


def test_box_coder_oracle_equals_float64():
    rng = np.random.default_rng(602)
    for axis, rows, cols in ((0, 3, 65), (1, 5, 7), (0, 1, 1)):
        m = cols if axis == 0 else rows
        lo = rng.random((m, 2)).astype(F32)
        prior = np.concatenate([lo, lo + F32(0.05) + rng.random((m, 2)).astype(F32) * F32(0.3)], axis=1)
        pvar = (0.05 + 0.3 * rng.random((m, 4))).astype(F32)
        target = rng.standard_normal((rows, cols, 4)).astype(F32)
        for kw in ({"prior_var": pvar}, {"variance": [0.1, 0.1, 0.2, 0.2]}, {}):
            for normalized in (True, False):
                got = D.box_coder_decode(prior, target, axis=axis, normalized=normalized, **kw)
                want = D.box_coder_decode(prior, target, axis=axis, normalized=normalized, dtype=np.float64, **kw)
                assert got.dtype == F32 and got.shape == target.shape
                # about 8 roundings of values bounded by the largest output
                assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max())), (axis, kw.keys(), normalized)
    # by hand: prior [0, 0, 2, 4], no variance, target 0: the prior itself; normalized off: widths + 1, far corner - 1
    p = np.array([[0, 0, 2, 4]], F32)
    assert np.array_equal(D.box_coder_decode(p, np.zeros((1, 1, 4), F32)), p[None])
    assert np.array_equal(D.box_coder_decode(p, np.zeros((1, 1, 4), F32), normalized=False), p[None])
    t = np.array([[[1, 1, 0, 0]]], F32)
    assert np.array_equal(D.box_coder_decode(p, t, variance=[0.5, 0.25, 1, 1]), np.array([[[1, 1, 3, 5]]], F32))


# ------------------------------------------------------------------ the corner rules
@pytest.mark.parametrize("name", sorted(D.corner_cases()))
def test_nms_corner_rule(name):
    boxes, scores, params, expected = D.corner_cases()[name]
    rows, offsets, index = D.multiclass_nms(boxes, scores, **params)
    assert index.tolist() == expected, name
    assert _same((rows, offsets, index), D.multiclass_nms_matrix(boxes, scores, **params)), name
    p = boxes.shape[1]
    for r, i in zip(rows, index):
        img, prior = divmod(int(i), p)
        assert np.array_equal(r[2:], boxes[img, prior]) and r[1].tobytes() == scores[img, int(r[0]), prior].tobytes()
        assert offsets[img] <= np.nonzero(index == i)[0][0] < offsets[img + 1] or (index == i).sum() > 1


def test_nms_corner_rule_details():
    cases = D.corner_cases()
    b, s, prm, _ = cases["signed_zero_scores"]
    rows, _o, _i = D.multiclass_nms(b, s, **prm)
    assert np.signbit(rows[:, 1]).tolist() == [True, False, True]          # the scores' own bits reach the rows
    b, s, prm, _ = cases["equal_scores_keep_top_k"]
    assert D.multiclass_nms(b, s, **prm)[0][:, 0].tolist() == [1, 1, 1]     # the cut keeps the lower label
    b, s, prm, _ = cases["no_detection_in_one_image"]
    assert D.multiclass_nms(b, s, **prm)[1].tolist() == [0, 0, 3]
    with pytest.raises(ValueError, match="nms_eta"):
        D.multiclass_nms(b, s, nms_eta=0.9, **prm)
    assert float(D.jaccard_overlap(np.array([0, 0, 2, 2], F32), np.array([0, 0, 2, 1], F32), True)) == 0.5
    assert np.isnan(D.jaccard_overlap(np.array([1, 1, 1, 1], F32), np.array([1, 1, 1, 1], F32), True))
    assert float(D.jaccard_overlap(np.array([0, 0, 1, 1], F32), np.array([3, 3, 4, 4], F32), False)) == 0.0


def test_padded_and_lod_forms():
    """detections_lod on hand-made padded arrays, and padded() as its inverse on an oracle result."""
    out = np.full((3, 2, 6), -1, F32)
    out[0, 0] = [1, 0.9, 0, 0, 1, 1]
    out[2, 0] = [2, 0.8, 1, 1, 2, 2]
    out[2, 1] = [3, 0.7, 2, 2, 3, 3]
    index = np.array([[4, -1], [-1, -1], [21, 25]], np.int32)
    rows, offsets, idx = D.detections_lod(out, [1, 0, 2], index)
    assert rows.tolist() == [out[0, 0].tolist(), out[2, 0].tolist(), out[2, 1].tolist()]
    assert offsets.tolist() == [0, 1, 1, 3] and idx.tolist() == [[4], [21], [25]]
    assert D.detections_lod(out, [1, 0, 2])[2] is None
    # no detection at all: [[-1]] with offsets [0, 1] without an index output, [0, 6] and [0, 1] with one
    rows, offsets, idx = D.detections_lod(np.full((2, 2, 6), -1, F32), [0, 0])
    assert rows.tolist() == [[-1.0]] and offsets.tolist() == [0, 1] and idx is None
    rows, offsets, idx = D.detections_lod(np.full((2, 2, 6), -1, F32), [0, 0], np.full((2, 2), -1, np.int32))
    assert rows.shape == (0, 6) and offsets.tolist() == [0, 0, 0] and idx.shape == (0, 1)
    boxes, scores, params, (r, o, i, _stats) = D.random_case((2, 3, 65))
    po, pc, pi = D.padded(r, o, i, params["keep_top_k"])
    assert po.shape == (2, params["keep_top_k"], 6) and pc.tolist() == np.diff(o).tolist()
    back = D.detections_lod(po, pc, pi)
    assert _same((r, o, i[:, None]), back)
    for k in range(2):
        assert (po[k, pc[k]:] == -1).all() and (pi[k, pc[k]:] == -1).all()


def test_transpose_and_reshape_rules():
    x = np.arange(2 * 3 * 5 * 7, dtype=F32).reshape(2, 3, 5, 7)
    for perm in itertools.permutations(range(4)):
        y = D.transpose(x, perm)
        assert y.flags.c_contiguous and y.shape == tuple(x.shape[k] for k in perm)
        o = tuple(d - 1 - (k == 2) for k, d in enumerate(y.shape))  # an output index; axis k of y is axis perm[k] of x
        src = [0] * 4
        for k in range(4):
            src[perm[k]] = o[k]
        assert y[o] == x[tuple(src)]
    for bad in ((0, 1, 2), (0, 1, 2, 2), (0, 1, 2, 4)):
        with pytest.raises(ValueError):
            D.transpose(x, bad)
    assert D.reshape_dims([2, 3, 5, 7], [0, -1, 7]) == [2, 15, 7]
    assert D.reshape_dims([2, 3, 5, 7], [0, 0, 35]) == [2, 3, 35]
    assert D.reshape_dims([6], [2, 3]) == [2, 3]
    for bad in ([-1, -1, 7], [0, -1, 4], [2, 3, 5], [0, 0, 0, 0, 0], [2, -2, 3]):
        with pytest.raises(ValueError):
            D.reshape_dims([2, 3, 5, 7], bad)
    a, b = x, np.arange(2 * 6 * 2 * 2, dtype=F32).reshape(2, 6, 2, 2)
    y = D.concat_nhwc([a, b], 3)
    assert y.shape == (2, 35 + 8, 3)
    assert np.array_equal(y[1, :35].reshape(5, 7, 3), x[1].transpose(1, 2, 0))


# ------------------------------------------------------------------ exports, refusals that need no device
def test_new_symbols_are_exported(pkg):
    capi = pkg.capi
    L = capi.load()
    text = open(os.path.join(ROOT, "include", "plhip.h")).read()
    for name in NEW_SYMBOLS + ("plhip_multiclass_nms_workspace_bytes",):
        assert name in capi.EXPORTS and hasattr(L, name), name
    for name in NEW_SYMBOLS:
        assert re.search(r"plhip_status %s\(plhip_ctx\* ctx" % name, text), name
    assert "size_t plhip_multiclass_nms_workspace_bytes(const plhip_nms_desc* desc);" in text
    for helper in ("transpose", "concat_nhwc", "box_coder_decode", "multiclass_nms"):
        assert hasattr(capi.Context, helper), helper
    # a NULL context is refused with the entry point's own text
    assert L.plhip_transpose_f32(None, None, None, None, 2, None) < 0
    assert L.plhip_last_error(None).decode().startswith("plhip_transpose_f32: ")
    assert L.plhip_concat_nhwc_f32(None, None, None, None, 1, 1, None) < 0
    assert L.plhip_last_error(None).decode().startswith("plhip_concat_nhwc_f32: ")
    assert L.plhip_box_coder_decode_f32(None, None, None, None, None, 1, 1, 0, 1, None) < 0
    assert L.plhip_last_error(None).decode().startswith("plhip_box_coder_decode_f32: ")
    assert L.plhip_multiclass_nms_f32(None, None, None, None, None, None, None, None) < 0
    assert L.plhip_last_error(None).decode().startswith("plhip_multiclass_nms_f32: ")


def test_nms_descriptor_layout_and_envelope(pkg):
    """plhip_nms_desc as ctypes lays it out equals the header's field order; the workspace query refuses what the entry point
    refuses (host logic) and sizes the two networks named in the header."""
    capi = pkg.capi
    L = capi.load()
    text = open(os.path.join(ROOT, "include", "plhip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} plhip_nms_desc;", text).group(1)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(" ", 1)[1].split(",")]
    assert fields == [f[0] for f in capi.NmsDesc._fields_]

    def ws(n, c, p, **kw):
        args = dict(background_label=0, score_threshold=0.01, nms_top_k=400, nms_threshold=0.45, keep_top_k=200)
        args.update(kw)
        return L.plhip_multiclass_nms_workspace_bytes(C.byref(capi.nms_desc(n, c, p, **args)))

    def refused(text_part, *a, **kw):
        assert ws(*a, **kw) == 0
        msg = L.plhip_last_error(None).decode()
        assert msg.startswith("plhip_multiclass_nms_workspace_bytes: ") and text_part in msg, msg

    assert ws(32, 21, 1917) == 32 * 21 * 200 * 8 + 32 * 21 * 4 + 16                      # SSD300
    assert ws(8, 80, 10647, nms_top_k=1000, keep_top_k=100) == 8 * 80 * 100 * 8 + 8 * 80 * 4 + 16  # YOLOv3-416
    assert ws(1, 2, 16384, nms_top_k=4096, keep_top_k=4096) > 0
    assert ws(1, 16385, 5, nms_top_k=1, keep_top_k=9) > 0 and ws(1, 16384, 5, nms_top_k=1, keep_top_k=9, background_label=-1) > 0
    refused("nms_eta", 1, 21, 1917, nms_eta=0.9)
    refused("keep_top_k", 1, 21, 1917, keep_top_k=-1)
    refused("keep_top_k", 1, 21, 1917, keep_top_k=0)
    refused("16384 priors", 1, 21, 16385)
    refused("4096", 1, 2, 5000, nms_top_k=-1)
    refused("4096", 1, 2, 5000, nms_top_k=4097)
    refused("above 16384", 1, 84, 1917)              # 83 * 200 > 16384
    refused("above 16384", 1, 16385, 5, nms_top_k=1, keep_top_k=9, background_label=-1)
    refused("at least 1", 0, 21, 1917)
    refused("65535", 65536, 2, 4)
    d = capi.nms_desc(1, 3, 7, 0, 0.01, 400, 0.45, 200)
    d.score_stride_class = 8
    assert L.plhip_multiclass_nms_workspace_bytes(C.byref(d)) == 0 and "strides" in L.plhip_last_error(None).decode()
    d = capi.nms_desc(1, 3, 7, 0, 0.01, 400, 0.45, 200, layout="npc")
    assert (d.score_stride_class, d.score_stride_prior) == (1, 3) and L.plhip_multiclass_nms_workspace_bytes(C.byref(d)) > 0
    assert L.plhip_multiclass_nms_workspace_bytes(None) == 0


# ------------------------------------------------------------------ the kept ISA
def _kernels(text):
    """name -> body of every kernel in a kept .s file."""
    out = {}
    for m in re.finditer(r"^(_ZN5plhip\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        out[m.group(1)] = m.group(2)
    return out


def test_kept_isa_has_no_scratch_and_no_contraction():
    """The ISA the build keeps beside detection_ops.o: box_coder_decode_kernel, nms_class_kernel and nms_image_kernel; none with a
    private segment; no fused or packed fp32 arithmetic in any (every product, sum and quotient of the decode and of the overlap
    rounds on its own; the only fused operations are those of the IEEE division sequence and of expf, which v_div_* and the
    library bring: the overlap's own products are v_mul_f32); LDS in the two NMS kernels only."""
    files = glob.glob(os.path.join(LITE, "csrc", "detection_ops-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert len(files) == 1, "build the library first (the ISA is kept beside the object)"
    text = open(files[0]).read()
    meta = re.findall(r"\.name:\s+(_ZN5plhip\S+)\n(?:(?!\s+\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    names = sorted(m[0] for m in meta)
    assert len(names) == 3 and len(set(names)) == 3, names
    assert sum("23box_coder_decode_kernel" in n for n in names) == 1 and sum("16nms_class_kernel" in n for n in names) == 1
    assert sum("16nms_image_kernel" in n for n in names) == 1
    assert all(size == "0" for _, size in meta), meta
    bodies = _kernels(text)
    assert sorted(bodies) == names
    for name, body in bodies.items():
        ops = set(re.findall(r"^\s+([a-z]\w+)", body, re.M))
        assert not [o for o in ops if o.startswith(("scratch_", "flat_"))], name
        assert not sorted(o for o in ops if re.match(r"v_pk_\w+_f32|v_dot", o)), name
        assert any(o.startswith("ds_") for o in ops) == ("nms" in name), name
        assert not [o for o in ops if "atomic" in o], name
    # The only fused operations are the library's: an IEEE division is 2 v_div_scale + v_rcp + at most 6 fused steps + v_div_fmas +
    # v_div_fixup, an expf 3 fused steps of its range reduction around one v_exp_f32.  Nothing of the decode or the overlap fuses.
    for name, body in bodies.items():
        ops = re.findall(r"^\s+([a-z]\w+)", body, re.M)
        fused = [o for o in ops if re.match(r"v_(fma|fmac|mac|mad)_f", o)]
        divs = sum(o.startswith("v_div_scale_f32") for o in ops) // 2
        exps = sum(o.startswith("v_exp_f32") for o in ops)
        assert len(fused) <= 6 * divs + 3 * exps, (name, fused, divs, exps)
        assert (divs, exps) == {"box_coder": (0, 2), "nms_class": (1, 0), "nms_image": (0, 0)}[re.search(r"box_coder|nms_class|nms_image", name).group(0)], name
        if "nms_image" not in name:
            assert "v_mul_f32_e32" in ops or "v_mul_f32_e64" in ops, name
