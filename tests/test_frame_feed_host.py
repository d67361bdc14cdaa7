"""Camera / decoder frames as input (image_convert + image_resize in front of image_to_tensor): the host side, checked without a
device.

The numpy restatements below restate the LIBRARY code the reference runs for ImagePreprocess::imageConvert and imageResize
(lite/utils/cv/paddle_image_preprocess.cc:44-98), not its test helper lite/tests/cv/cv_basic.h, which differs:

* nv_to_bgr_ref: lite/utils/cv/image_convert.cc:175-518; the scalar tail :451-514 states the arithmetic, the NEON body :242-449
  computes the same values in int16 without overflow (|227 * 128| < 2^15), so there is one answer;
* resize_tables_ref: the table part of lite/utils/cv/image_resize.cc (:184-259 one channel, the same lines at :564- and :728-):
  a double expression rounded ONCE to float, floor, a float subtract, two clamps, SATURATE_CAST_SHORT;
* image_resize_ref: the row / column passes of image_resize.cc:184-369 (one channel), :564-726 (three), :728-895 (four), dispatch
  :897-926 (equal sizes: a copy).  a0 + a1 is 2048, or 2049 at a rounding tie; with both weight sums <= 2049 every result is in
  0..255 (2049 * 32655 >> 16 = 1020, (1020 + 2) >> 2 = 255, every term non-negative), so the NEON path's saturating narrow
  (vqmovun_s16) and the scalar tail's (uint8_t) cast agree and the result does not depend on w_out % 8: one answer.  The bound is
  asserted on the restatement's intermediates (test_restatement_bounds).

Every comparison of this feature is exact; there is no tolerance anywhere.
"""
import ctypes
import importlib

import numpy as np
import pytest

from test_image_feed_host import BGR, BGRA, GRAY, MEANS, PIXEL_BYTES, RGB, RGBA, SCALES

NV21, NV12 = 11, 12  # cv::ImageFormat, lite/utils/cv/cv_enum.h:21-29
EXTREMES = (0, 1, 127, 128, 129, 254, 255)


def nv_to_bgr_ref(frame, nv21):
    """uint8 [n, h * 3 / 2, w] -> uint8 [n, h, w, 3] (b, g, r).  C integer arithmetic: numpy's >> on negative int32 is arithmetic."""
    frame = np.asarray(frame, np.uint8)
    n, rows, w = frame.shape
    h = rows // 3 * 2
    assert rows * 2 == h * 3 and h % 2 == 0 and w % 2 == 0
    y = frame[:, :h].astype(np.int32)
    pairs = frame[:, h:].reshape(n, h // 2, w // 2, 2).astype(np.int32)
    u, v = (pairs[..., 1], pairs[..., 0]) if nv21 else (pairs[..., 0], pairs[..., 1])
    u = np.repeat(np.repeat(u, 2, axis=1), 2, axis=2) - 128  # one pair per 2 x 2 luma block
    v = np.repeat(np.repeat(v, 2, axis=1), 2, axis=2) - 128
    ra = (179 * v) >> 7
    ga = (44 * u + 91 * v) >> 7
    ba = (227 * u) >> 7
    return np.stack([np.clip(y + ba, 0, 255), np.clip(y - ga, 0, 255), np.clip(y + ra, 0, 255)], axis=-1).astype(np.uint8)


def resize_tables_ref(n_in, n_out):
    """(ofs int32 [n_out], coef int16 [n_out, 2]) of one axis."""
    assert n_in >= 2 and n_out >= 1
    scale = float(n_in) / n_out                                          # double
    d = np.arange(n_out, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)                     # double expression, ONE rounding to float
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)                                         # float subtract
    lo, hi = s < 0, s >= n_in - 1
    s = np.where(lo, 0, s)
    f = np.where(lo, np.float32(0), f)
    s = np.where(hi, n_in - 2, s).astype(np.int32)
    f = np.where(hi, np.float32(1), f).astype(np.float32)

    def sat_short(x):  # (int)(X + (X >= 0 ? 0.5f : -0.5f)) clamped to int16; the cast truncates towards zero
        x = x.astype(np.float32)
        r = (x + np.where(x >= 0, np.float32(0.5), np.float32(-0.5)).astype(np.float32)).astype(np.float32)
        return np.clip(np.trunc(r).astype(np.int64), -32768, 32767).astype(np.int16)

    coef = np.stack([sat_short((np.float32(1) - f) * np.float32(2048)), sat_short(f * np.float32(2048))], axis=-1)
    return s, coef


def image_resize_ref(src, h_out, w_out, stats=None):
    """uint8 [n, h, w, cs] -> uint8 [n, h_out, w_out, cs], every byte of a pixel alike.  stats: a dict that receives the largest
    `rows` intermediate and the smallest / largest result BEFORE the cast to uint8."""
    src = np.asarray(src, np.uint8)
    n, h, w, cs = src.shape
    if (h, w) == (h_out, w_out):
        return src.copy()  # image_resize.cc:905-915
    sx, ca = resize_tables_ref(w, w_out)
    sy, cb = resize_tables_ref(h, h_out)
    a0, a1 = ca[:, 0].astype(np.int32)[None, None, :, None], ca[:, 1].astype(np.int32)[None, None, :, None]
    b0, b1 = cb[:, 0].astype(np.int32)[None, :, None, None], cb[:, 1].astype(np.int32)[None, :, None, None]
    s = src.astype(np.int32)
    top, bot = s[:, sy], s[:, sy + 1]
    rows0 = (top[:, :, sx] * a0 + top[:, :, sx + 1] * a1) >> 4
    rows1 = (bot[:, :, sx] * a0 + bot[:, :, sx + 1] * a1) >> 4
    dst = (((b0 * rows0) >> 16) + ((b1 * rows1) >> 16) + 2) >> 2
    if stats is not None:
        stats["rows_max"] = max(stats.get("rows_max", 0), int(rows0.max()), int(rows1.max()))
        stats["dst_min"] = min(stats.get("dst_min", 0), int(dst.min()))
        stats["dst_max"] = max(stats.get("dst_max", 0), int(dst.max()))
    return dst.astype(np.uint8)


def extremes_frame(nv21):
    """One NV frame [1, 21, 98] (h 14, w 98) whose 2 x 2 blocks run through (y, u, v) in EXTREMES^3 (343 blocks, 7 x 49)."""
    h, w = 14, 98
    f = np.zeros((1, h * 3 // 2, w), np.uint8)
    i = 0
    for yv in EXTREMES:
        for u in EXTREMES:
            for v in EXTREMES:
                r, c = i // 49, i % 49
                f[0, 2 * r:2 * r + 2, 2 * c:2 * c + 2] = yv
                f[0, h + r, 2 * c:2 * c + 2] = (v, u) if nv21 else (u, v)
                i += 1
    return f


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


TABLE_CASES = [(1920, 224), (1080, 224), (640, 224), (480, 224), (256, 224), (80, 224), (2, 7), (3, 2), (224, 224), (2, 5), (37, 33),
               (53, 223), (100, 224), (720, 224), (1280, 224)]


def test_resize_tables_equal_restatement(pkg):
    """plhip_image_resize_tables (host only) == resize_tables_ref; 1920 -> 224 and 1080 -> 224 really contain rounding ties
    (a0 + a1 == 2049), and both clamps occur when upscaling."""
    capi = pkg.capi
    for (n_in, n_out) in TABLE_CASES:
        ofs, coef = capi.resize_tables(n_in, n_out)
        rofs, rcoef = resize_tables_ref(n_in, n_out)
        assert np.array_equal(ofs, rofs) and np.array_equal(coef, rcoef), (n_in, n_out)
        sums = coef.astype(np.int32).sum(axis=1)
        assert set(np.unique(sums)) <= {2048, 2049}, (n_in, n_out, np.unique(sums))
        assert ofs.min() >= 0 and ofs.max() <= n_in - 2
        if (n_in, n_out) in ((1920, 224), (1080, 224)):
            assert (sums == 2049).any(), (n_in, n_out)
        if (n_in, n_out) in ((256, 224), (80, 224)):
            assert not (sums == 2049).any(), (n_in, n_out)
    for (n_in, n_out) in ((80, 224), (2, 7)):  # upscaling: the first output falls left of the source (sx < 0), the last right of it
        d = np.arange(n_out, dtype=np.float64)
        f = ((d + 0.5) * (float(n_in) / n_out) - 0.5).astype(np.float32)
        raw = np.floor(f).astype(np.int64)
        assert (raw < 0).any() and (raw >= n_in - 1).any()
        ofs, coef = capi.resize_tables(n_in, n_out)
        assert tuple(coef[0]) == (2048, 0) and ofs[0] == 0
        assert tuple(coef[-1]) == (0, 2048) and ofs[-1] == n_in - 2
    # refused, no abort: a source of fewer than 2, no output, null pointers
    assert capi.resize_tables(1, 5) is None and capi.resize_tables(0, 5) is None and capi.resize_tables(5, 0) is None
    assert capi.load().plhip_image_resize_tables(4, 4, None, None) != 0


def test_restatement_bounds():
    """rows <= 32655 (fits int16) and results in 0..255 before the cast, on an all-255 and a random frame, through sizes with ties."""
    rng = np.random.default_rng(11)
    stats = {}
    for (h, w, ho, wo) in ((1080, 1920, 224, 224), (80, 100, 224, 224), (37, 53, 33, 223), (2, 2, 5, 7)):
        full = np.full((1, h, w, 3), 255, np.uint8)
        assert (image_resize_ref(full, ho, wo, stats) == 255).all()
        image_resize_ref(rng.integers(0, 256, (1, h, w, 4)).astype(np.uint8), ho, wo, stats)
    assert stats["rows_max"] <= 32655 and stats["dst_min"] >= 0 and stats["dst_max"] <= 255, stats
    assert stats["rows_max"] == 32655 and stats["dst_max"] == 255  # the tie 2049 * 255 >> 4 is reached
    # equal sizes: a copy; and the general formula itself is the identity there (what the fused NV kernel relies on)
    x = rng.integers(0, 256, (2, 6, 8, 3)).astype(np.uint8)
    assert np.array_equal(image_resize_ref(x, 6, 8), x)
    ofs, coef = resize_tables_ref(8, 8)
    assert np.array_equal(ofs, [0, 1, 2, 3, 4, 5, 6, 6]) and tuple(coef[-1]) == (0, 2048) and (coef[:-1] == (2048, 0)).all()


def test_nv_restatement_extremes():
    """(y, u, v) over EXTREMES^3 hits both clamps of every colour; hand-computed pixels; NV12 and NV21 differ by the pair's order."""
    for nv21 in (False, True):
        out = nv_to_bgr_ref(extremes_frame(nv21), nv21)
        assert out.shape == (1, 14, 98, 3)
        for c in range(3):
            assert (out[..., c] == 0).any() and (out[..., c] == 255).any(), c
    assert np.array_equal(nv_to_bgr_ref(extremes_frame(False), False), nv_to_bgr_ref(extremes_frame(True), True))
    # y 100, u 255, v 0: ra = (179 * -128) >> 7 = -179, ga = (44 * 127 + 91 * -128) >> 7 = -6060 >> 7 = -48, ba = (227 * 127) >> 7 = 225
    f = np.array([[[100, 100], [100, 100], [255, 0]]], np.uint8)
    assert nv_to_bgr_ref(f, False)[0, 0, 0].tolist() == [255, 148, 0]
    # the same bytes read as NV21: u 0, v 255: ra = 177, ga = (44 * -128 + 91 * 127) >> 7 = 5925 >> 7 = 46, ba = -227
    assert nv_to_bgr_ref(f, True)[0, 1, 1].tolist() == [0, 54, 255]
    # u = v = 128: grey
    g = np.array([[[7, 200], [0, 255], [128, 128]]], np.uint8)
    assert nv_to_bgr_ref(g, False)[0].tolist() == [[[7] * 3, [200] * 3], [[0] * 3, [255] * 3]]


def test_new_exports_and_constants(pkg, lite):
    capi = pkg.capi
    L = capi.load()
    for sym in ("plhip_image_resize_tables", "plhip_image_convert_u8", "plhip_image_resize_u8", "plhip_frame_to_tensor_f32",
                "plhip_frame_to_tensor_i8"):
        assert hasattr(L, sym) and sym in capi.EXPORTS, sym
    assert hasattr(lite.load(), "pllite_graph_feed_frame")
    assert (capi.IMG_NV21, capi.IMG_NV12) == (lite.IMG_NV21, lite.IMG_NV12) == (NV21, NV12)
    assert ctypes.sizeof(capi.FrameDesc) == 16
    for op, aliases in (("image_convert", 1), ("image_resize", 3)):
        assert lite.load().pllite_registered_kernels(op.encode(), lite.PREC_ANY, lite.LAYOUT_NCHW) == aliases, op


def _plan(lite, wl, net, batch=2, fuse=True, image=None, frame=None):
    p = lite.Predictor(planner=True)
    try:
        wl.emit_graph(p, net, batch, fuse=fuse, image=image, frame=frame)
        return p.graph_plan()
    finally:
        p.close()


IMAGE = dict(format=BGR, means=MEANS, scales=SCALES)


def _frame(h, w, fmt):
    return dict(h=h, w=w, format=fmt, means=MEANS, scales=SCALES)


def test_mobilenet_v1_nv12_frame_plans(lite, wl):
    """1080 x 1920 NV12 -> 224 x 224.  Unfused: io_copy -> image_convert -> image_resize -> image_to_tensor -> calib -> the stem.
    Fused (I): ONE image_resize/int8 instruction reading the NV12 frame, then the stem on the int8 tensor: 20 instructions."""
    net = wl.mobilenet_v1_net()
    fr = _frame(1080, 1920, NV12)
    off, off_f32 = _plan(lite, wl, net, fuse=False, frame=fr), _plan(lite, wl, net, fuse=False)
    assert off[0] == "io_copy/host_to_device in=image out=image/target_trans"
    assert off[1] == "image_convert/def in=image/target_trans out=image/bgr src=NV12 dst=BGR"
    assert off[2] == "image_resize/uint8 in=image/bgr out=image/image src=BGR 1080x1920->224x224"
    assert off[3] == "image_to_tensor/fp32 in=image/image out=image/tensor fmt=BGR"
    assert off[4].startswith("calib/fp32_to_int8 in=image/tensor out=image/precision_trans scale=")
    assert off[5].startswith("conv2d/int8_out in=image/precision_trans out=conv1 ")
    assert len(off) == len(off_f32) + 3 and off[5:] == off_f32[2:]
    for batch in (2, 128):
        on, on_f32 = _plan(lite, wl, net, batch, frame=fr), _plan(lite, wl, net, batch)
        assert len(on) == 20 and len(on_f32) == 19
        assert on[1].startswith("image_resize/int8 in=image/target_trans out=image/precision_trans src=NV12 1080x1920->224x224 scale=")
        assert on[2].startswith("conv2d/int8_out in=image/precision_trans out=conv1 ") and "+image_in" not in on[2] and "+calib_in" not in on[2]
        assert on[3:] == on_f32[2:]
        assert not any("image_convert" in l or "image_to_tensor" in l for l in on)
    nv21 = _plan(lite, wl, net, frame=_frame(480, 640, NV21))
    assert " src=NV21 480x640->224x224 scale=" in nv21[1]


def test_resnet50_bgr_frame_plans(lite, wl):
    """480 x 640 BGR -> the net's 64 x 64: no convert; fused, image_resize/int8 stands where the image feed has image_to_tensor/int8."""
    r50 = wl.resnet50_net(res=64)
    fr = _frame(480, 640, BGR)
    on, img = _plan(lite, wl, r50, frame=fr), _plan(lite, wl, r50, image=IMAGE)
    assert len(on) == len(img)
    assert on[1].startswith("image_resize/int8 in=image/target_trans out=image/precision_trans src=BGR 480x640->64x64 scale=")
    assert on[1].split(" scale=")[1] == img[1].split(" scale=")[1]
    assert on[0] == img[0] and on[2:] == img[2:]
    off = _plan(lite, wl, r50, fuse=False, frame=fr)
    assert off[1] == "image_resize/uint8 in=image/target_trans out=image/image src=BGR 480x640->64x64"
    assert off[2] == "image_to_tensor/fp32 in=image/image out=image/tensor fmt=BGR"
    assert off[3:] == _plan(lite, wl, r50, fuse=False, image=IMAGE)[2:]


def test_equal_size_frame_is_an_image_feed_and_image_feeds_are_unchanged(lite, wl):
    """A frame feed of the network's size in an interleaved format lowers byte for byte like FeedImage (H1 / H2 included); an NV
    frame of the network's size keeps its convert as a launch and image_to_tensor (then H) behind it; FeedImage plans themselves
    do not notice the feature (generated here from FeedImage, with and without the new keyword)."""
    for net in (wl.mobilenet_v1_net(), wl.resnet50_net(res=64)):
        c, h, w = net["input_shape"]
        for fuse in (True, False):
            img = _plan(lite, wl, net, fuse=fuse, image=IMAGE)
            assert _plan(lite, wl, net, fuse=fuse, frame=_frame(h, w, BGR)) == img
            assert _plan(lite, wl, net, fuse=fuse, image=IMAGE, frame=None) == img
            assert not any("image_resize" in l or "image_convert" in l for l in img)
    net = wl.mobilenet_v1_net()
    nv = _plan(lite, wl, net, frame=_frame(224, 224, NV12))
    img = _plan(lite, wl, net, image=IMAGE)
    assert nv[1] == "image_convert/def in=image/target_trans out=image/bgr src=NV12 dst=BGR"
    assert nv[2].startswith("conv2d/int8_out in=image/bgr out=conv1 ") and " +image_in=image fmt=BGR " in nv[2]
    assert len(nv) == len(img) + 1 and nv[3:] == img[2:]


def test_refusals(lite, wl):
    """Odd NV sizes, a source of fewer than 2 rows / columns, NV into FeedImage, an unknown format: LiteError, no abort."""
    m, s = MEANS, SCALES

    def feed(fn):
        p = lite.Predictor(planner=True)
        try:
            fn(p)
        finally:
            p.close()

    for (sh, sw) in ((481, 640), (480, 641)):
        with pytest.raises(lite.LiteError):
            feed(lambda p: p.graph_feed_frame("image", 1, sh, sw, NV12, 224, 224, m, s))
    for (sh, sw) in ((1, 640), (480, 1)):
        with pytest.raises(lite.LiteError):
            feed(lambda p: p.graph_feed_frame("image", 1, sh, sw, BGR, 224, 224, m, s))
    for fmt in (NV12, NV21):
        with pytest.raises(lite.LiteError):
            feed(lambda p: p.graph_feed_image("image", 1, 224, 224, fmt, m, s))
    for fmt in (5, 10, 13, -1):
        with pytest.raises(lite.LiteError):
            feed(lambda p: p.graph_feed_frame("image", 1, 480, 640, fmt, 224, 224, m, s))
    feed(lambda p: p.graph_feed_frame("image", 1, 480, 641, BGR, 224, 224, m, s))  # odd sizes are fine for interleaved frames
    # the C ABI refuses before it touches a device: null context / pointers give a status
    capi = importlib.import_module("paddle_lite_amd.capi")
    L = capi.load()
    f = capi.frame_desc(1, 480, 640, capi.IMG_NV12)
    assert L.plhip_image_convert_u8(None, ctypes.byref(f), None, capi.IMG_BGR, None) == -1
    assert L.plhip_image_resize_u8(None, ctypes.byref(f), None, 224, 224, None) == -1
    img = capi.image_desc(1, 224, 224, capi.IMG_BGR, m, s)
    assert L.plhip_frame_to_tensor_f32(None, ctypes.byref(f), ctypes.byref(img), None, None) == -1
    assert L.plhip_frame_to_tensor_i8(None, ctypes.byref(f), ctypes.byref(img), None, None, 0.01) == -1
