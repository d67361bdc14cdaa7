"""CPU: yolo_oracle pinned without the device.  The float32 oracle against the independent float64 evaluation within the derived
bounds (the reference's own function does not compile on an x86 host, see yolo_oracle's head), hand-computed cells including the
grid_size = h quirk on a 2 x 6 map, the skip / NaN / clip rules, the head's composition, and the Python bindings of the two C ABI
entry points."""
import numpy as np
import pytest

import yolo_oracle as Y

F32 = np.float32
A3 = [10, 13, 16, 30, 33, 23]


@pytest.mark.parametrize("h,w", [(4, 4), (3, 3), (2, 6), (13, 13)])
@pytest.mark.parametrize("clip,sxy,thresh", [(True, 1.0, 0.5), (False, 1.05, 0.5), (True, 1.05, 0.0), (False, 1.0, 1.5)])
def test_oracle_against_the_float64_evaluation(h, w, clip, sxy, thresh):
    n, c = 2, 3
    x = Y.random_map(6000 + 16 * h + w, n, 3, c, h, w)
    img = Y.random_img_size(6001, n)
    boxes, scores, pt = Y.yolo_box(x, img, A3, c, thresh, 32, clip, sxy, parts=True)
    b64, s64 = Y.yolo_box_f64(x, img, A3, c, thresh, 32, clip, sxy)
    assert boxes.shape == (n, 3 * h * w, 4) and scores.shape == (n, 3 * h * w, c) and boxes.dtype == F32 and scores.dtype == F32
    worst = Y.check_against(boxes, scores, b64.astype(F32), s64.astype(F32), pt, "oracle vs float64")
    # and against the unrounded float64 values themselves: the float32 chain is a handful of roundings
    unit = Y.ULP * (np.abs(pt["centre"]) + np.abs(pt["half"])).astype(np.float64)
    assert (np.abs(boxes - b64) <= 8 * unit)[pt["keep"]].all()
    assert (np.abs(scores - s64) <= 8 * Y.ULP * s64).all()
    assert np.array_equal(scores == 0, s64 == 0) and np.array_equal((boxes == 0).all(-1) | pt["keep"], pt["keep"] | ~(b64 != 0).any(-1))
    assert worst[0] <= 8 and worst[1] <= 8


def test_hand_computed_cells_on_a_2x6_map():
    """All logits 0: sigmoid = 0.5, exp = 1.  h = 2 is the grid size of BOTH axes and the input size is 32 * 2 = 64, so with a
    640 x 480 (w x h) image cell (k 1, l 5) of anchor (16, 30) has cx = 5.5 * 640 / 2 = 1760 (outside the image: l / h, not l / w),
    cy = 1.5 * 480 / 2 = 360, bw = 16 * 640 / 64 = 160, bh = 30 * 480 / 64 = 225."""
    x = np.zeros((1, 3 * 8, 2, 6), F32)
    img = np.array([[480, 640]], np.int32)
    boxes, scores = Y.yolo_box(x, img, A3, 3, 0.5, 32, clip_bbox=False)
    idx = 1 * 12 + 1 * 6 + 5
    assert boxes[0, idx].tolist() == [1760 - 80, 360 - 112.5, 1760 + 80, 360 + 112.5]
    assert (scores == F32(0.25)).all()      # conf 0.5 is NOT below 0.5: kept
    clipped, _ = Y.yolo_box(x, img, A3, 3, 0.5, 32, clip_bbox=True)
    assert clipped[0, idx].tolist() == [1680.0, 247.5, 639.0, 472.5]   # only the far x corner passes img_w - 1
    # cell (0, 0) of anchor (10, 13): cx = 160, cy = 120, bw = 100, bh = 97.5
    assert boxes[0, 0].tolist() == [110.0, 71.25, 210.0, 168.75]
    # scale_x_y 1.05: bias = float(-0.5 * (double(1.05f) - 1)); cx = (0 + 0.5f * 1.05f + bias) * 640 / 2
    b2, _ = Y.yolo_box(x, img, A3, 3, 0.5, 32, clip_bbox=False, scale_x_y=1.05)
    bias = F32(-0.5 * (float(F32(1.05)) - 1.0))
    cx = (F32(0) + F32(0.5) * F32(1.05) + bias) * F32(640) / F32(2)
    assert b2[0, 0, 0] == cx - F32(50) and b2[0, 0, 2] == cx + F32(50)
    # just above the threshold everything is skipped: zeros, positive ones
    b3, s3 = Y.yolo_box(x, img, A3, 3, 0.5000001, 32)
    assert not b3.view(np.uint32).any() and not s3.view(np.uint32).any()


def test_nan_objectness_is_kept_and_the_clip_maps_nan():
    x = np.zeros((1, 8, 2, 2), F32)
    x[0, 4, 0, 0] = np.nan            # objectness of cell 0
    x[0, 0, 0, 1] = np.nan            # x of cell 1
    x[0, 4, 1, 1] = -5.0              # cell 3 falls below the threshold
    img = np.array([[100, 200]], np.int32)
    boxes, scores, pt = Y.yolo_box(x, img, [10, 13], 3, 0.3, 32, parts=True)
    assert pt["keep"].tolist() == [[True, True, True, False]]
    assert np.isnan(scores[0, 0]).all() and np.isfinite(boxes[0, 0]).all()
    assert boxes[0, 1, 0] == 0 and boxes[0, 1, 2] == 199 and np.isfinite(boxes[0, 1]).all()   # NaN > 0 and NaN < 199 are false
    assert not boxes[0, 3].any() and not scores[0, 3].any()
    raw, _ = Y.yolo_box(x, img, [10, 13], 3, 0.3, 32, clip_bbox=False)
    assert np.isnan(raw[0, 1, [0, 2]]).all() and np.isfinite(raw[0, 1, [1, 3]]).all()


def test_threshold_condition_is_asserted():
    x = np.zeros((1, 8, 1, 1), F32)
    pt = Y.yolo_box(x, np.array([[10, 10]], np.int32), [10, 13], 3, 0.5, 32, parts=True)[2]
    with pytest.raises(AssertionError, match="within 32 ulp"):
        Y.assert_clear_of_threshold(pt)
    Y.assert_clear_of_threshold(Y.yolo_box(x, np.array([[10, 10]], np.int32), [10, 13], 3, 0.0, 32, parts=True)[2])


def test_check_dims_messages():
    for args, part in ((((1, 24, 2), (1, 2), A3, 3), "rank 4"), (((1, 24, 2, 2), (1, 2), [], 3), "pairs"), (((1, 24, 2, 2), (1, 2), [1, 2, 3], 3), "pairs"),
                       (((1, 24, 2, 2), (1, 2), A3, 0), "class_num"), (((1, 25, 2, 2), (1, 2), A3, 3), "channels"),
                       (((2, 24, 2, 2), (1, 2), A3, 3), "ImgSize"), (((1, 24, 2, 2), (1, 3), A3, 3), "ImgSize")):
        with pytest.raises(ValueError, match=part):
            Y.check_dims(*args)


def test_head_is_the_composition():
    n, c = 2, 3
    maps = [(3, 3), (6, 6), (12, 12)]
    xs = [Y.random_map(6010 + i, n, 3, c, h, w) for i, (h, w) in enumerate(maps)]
    img = Y.random_img_size(6011, n)
    boxes, scores, pt = Y.yolo_head(xs, img, [A3] * 3, c, 0.5, [32, 16, 8], parts=True)
    assert boxes.shape == (n, 567, 4) and scores.shape == (n, c, 567) and pt["keep"].shape == (n, 567)
    b1, s1 = Y.yolo_box(xs[1], img, A3, c, 0.5, 16)
    assert np.array_equal(boxes[:, 27:27 + 108], b1) and np.array_equal(scores[:, :, 27:27 + 108], s1.transpose(0, 2, 1))


def test_bindings_exist(pkg):
    """The two entry points are declared in the header and bound in capi; neither exists before this feature."""
    import os
    import conftest
    header = open(os.path.join(conftest.ROOT, "include", "plhip.h")).read()
    for name in ("plhip_yolo_box_f32", "plhip_yolo_head_f32"):
        assert name in pkg.capi.EXPORTS
        assert "plhip_status %s(" % name in header
    for name in ("yolo_box", "yolo_head", "yolo_box_launch", "yolo_head_launch"):
        assert callable(getattr(pkg.capi.Context, name))
