"""Camera / decoder frames as input on the MI355X, all bit-exact: plhip_image_convert_u8, plhip_image_resize_u8 and
plhip_frame_to_tensor_f32 / _i8 against the numpy restatements of image_convert.cc / image_resize.cc / image2tensor.cc (+ the
oracle's calib) and against each other through the C ABI (three launches, two, one), and whole programs fed an NV12 frame batch
against the same program fed the restated uint8 image through the existing FeedImage path."""
import ctypes
import importlib

import numpy as np
import pytest

from test_frame_feed_host import NV12, NV21, extremes_frame, image_resize_ref, nv_to_bgr_ref
from test_image_feed_host import BGR, BGRA, GRAY, MEANS, PIXEL_BYTES, RGB, RGBA, SCALES, image_to_tensor_ref

pytestmark = pytest.mark.gpu

FORMATS = (RGBA, BGRA, RGB, BGR, GRAY)
CALIB = 1.0 / 127 * 1.1
# (h_in, w_in) -> (h_out, w_out)
RESIZES = (((1080, 1920), (224, 224)), ((480, 640), (224, 224)), ((256, 256), (224, 224)), ((80, 100), (224, 224)), ((2, 2), (5, 7)),
           ((37, 53), (33, 223)), ((224, 224), (224, 224)))


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _nv_frame(rng, n, h, w):
    return rng.integers(0, 256, (n, h * 3 // 2, w)).astype(np.uint8)


def test_image_convert(gpu_ctx, pkg):
    """NV12 and NV21, n in {1, 3}, the scalar form (2 x 2, 6 x 34) and the vector one (480 x 640), BGR and BGRA, the extremes."""
    capi = pkg.capi
    rng = np.random.default_rng(12)
    for fmt, nv21 in ((NV12, False), (NV21, True)):
        for n in (1, 3):
            for (h, w) in ((2, 2), (6, 34), (480, 640)):
                src = _nv_frame(rng, n, h, w)
                ref = nv_to_bgr_ref(src, nv21)
                got = gpu_ctx.image_convert(capi.frame_desc(n, h, w, fmt), src)
                assert got.shape == ref.shape and np.array_equal(got, ref), (fmt, n, h, w)
        ex = extremes_frame(nv21)
        assert np.array_equal(gpu_ctx.image_convert(capi.frame_desc(1, 14, 98, fmt), ex), nv_to_bgr_ref(ex, nv21))
        for (h, w) in ((6, 34), (32, 64)):
            src = _nv_frame(rng, 2, h, w)
            bgra = gpu_ctx.image_convert(capi.frame_desc(2, h, w, fmt), src, capi.IMG_BGRA)
            assert np.array_equal(bgra[..., :3], nv_to_bgr_ref(src, nv21)) and (bgra[..., 3] == 255).all()


def _frames(rng, n, h, w, cs):
    """random bytes, an all-255 frame and a 0 / 255 checkerboard"""
    yield "random", rng.integers(0, 256, (n, h, w, cs)).astype(np.uint8)
    yield "full", np.full((n, h, w, cs), 255, np.uint8)
    board = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
    yield "board", np.broadcast_to(board[None, :, :, None], (n, h, w, cs)).copy()


def test_image_resize_u8(gpu_ctx, pkg):
    capi = pkg.capi
    rng = np.random.default_rng(13)
    for fmt in FORMATS:
        cs = PIXEL_BYTES[fmt]
        for ((hi, wi), (ho, wo)) in RESIZES:
            for n in ((1,) if hi == 1080 else (1, 3)):
                for kind, src in _frames(rng, n, hi, wi, cs):
                    if kind != "random" and (n == 3 or hi == 1080):
                        continue
                    got = gpu_ctx.image_resize(capi.frame_desc(n, hi, wi, fmt), src, ho, wo)
                    ref = image_resize_ref(src, ho, wo)
                    assert got.shape == ref.shape and np.array_equal(got, ref), (fmt, n, hi, wi, ho, wo, kind, int((got != ref).sum()))


def test_frame_to_tensor(gpu_ctx, pkg, plref):
    """One launch == restatement of resize -> image_to_tensor (-> the oracle's calib), == the separate launches through the C ABI,
    w_out in {223, 224}: the scalar and the vector store paths."""
    capi = pkg.capi
    rng = np.random.default_rng(14)
    sizes = tuple(RESIZES) + (((480, 640), (224, 223)), ((80, 100), (37, 223)))
    for fmt in FORMATS:
        cs = PIXEL_BYTES[fmt]
        for ((hi, wi), (ho, wo)) in sizes:
            if hi == 1080 and fmt not in (BGR, RGBA):
                continue
            n = 1 if hi == 1080 else 2
            src = rng.integers(0, 256, (n, hi, wi, cs)).astype(np.uint8)
            fr, img = capi.frame_desc(n, hi, wi, fmt), capi.image_desc(n, ho, wo, fmt, MEANS, SCALES)
            small = image_resize_ref(src, ho, wo)
            ref = image_to_tensor_ref(small, fmt, MEANS, SCALES)
            y = gpu_ctx.frame_to_tensor(fr, img, src)
            assert y.dtype == np.float32 and np.array_equal(_bits(y), _bits(ref)), (fmt, hi, wi, ho, wo)
            q = gpu_ctx.frame_to_tensor(fr, img, src, CALIB)
            assert np.array_equal(q, plref.calib_f32_to_i8(ref, CALIB)), (fmt, hi, wi, ho, wo)
            # two launches through the C ABI: resize, then image_to_tensor
            dev_small = gpu_ctx.image_resize(fr, src, ho, wo)
            assert np.array_equal(_bits(gpu_ctx.image_to_tensor(img, dev_small)), _bits(y))
            assert np.array_equal(gpu_ctx.image_to_tensor(img, dev_small, CALIB), q)


def test_frame_to_tensor_nv_every_form(gpu_ctx, pkg, plref):
    """NV12 / NV21 sources: three launches (convert, resize, image_to_tensor), two (convert, fused resize + tensor; and fused
    convert + resize, image_to_tensor) and one, all equal to the restatement; an NV frame of the image's own size too."""
    capi = pkg.capi
    rng = np.random.default_rng(15)
    for fmt, nv21 in ((NV12, False), (NV21, True)):
        for ((hi, wi), (ho, wo)) in (((1080, 1920), (224, 224)), ((480, 640), (224, 224)), ((480, 640), (224, 223)), ((6, 34), (33, 48)),
                                     ((2, 2), (5, 7)), ((32, 64), (32, 64))):
            n = 1 if hi == 1080 else 3
            src = _nv_frame(rng, n, hi, wi)
            fr, bgr_fr = capi.frame_desc(n, hi, wi, fmt), capi.frame_desc(n, hi, wi, capi.IMG_BGR)
            img = capi.image_desc(n, ho, wo, capi.IMG_BGR, MEANS, SCALES)
            bgr_ref = nv_to_bgr_ref(src, nv21)
            small_ref = image_resize_ref(bgr_ref, ho, wo)
            ref = image_to_tensor_ref(small_ref, BGR, MEANS, SCALES)
            ref_q = plref.calib_f32_to_i8(ref, CALIB)
            one, one_q = gpu_ctx.frame_to_tensor(fr, img, src), gpu_ctx.frame_to_tensor(fr, img, src, CALIB)
            assert np.array_equal(_bits(one), _bits(ref)) and np.array_equal(one_q, ref_q), (fmt, hi, wi, ho, wo)
            bgr = gpu_ctx.image_convert(fr, src)
            small = gpu_ctx.image_resize(bgr_fr, bgr, ho, wo)
            assert np.array_equal(bgr, bgr_ref) and np.array_equal(small, small_ref)
            assert np.array_equal(gpu_ctx.image_resize(fr, src, ho, wo), small_ref)          # convert + resize fused
            assert np.array_equal(_bits(gpu_ctx.image_to_tensor(img, small)), _bits(one))    # three launches
            assert np.array_equal(gpu_ctx.image_to_tensor(img, small, CALIB), one_q)
            assert np.array_equal(_bits(gpu_ctx.frame_to_tensor(bgr_fr, img, bgr)), _bits(one))  # two launches
            assert np.array_equal(gpu_ctx.frame_to_tensor(bgr_fr, img, bgr, CALIB), one_q)


def test_frame_to_tensor_rounding_ties(gpu_ctx, pkg, plref):
    """The means / scales of test_image_to_tensor_rounding_ties: many normalised values on the calib's ties and past its bound."""
    capi = pkg.capi
    src = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3).copy()
    src[..., 1] = src[..., 1][:, ::-1]
    big = src.repeat(3, axis=1).repeat(2, axis=2)  # 48 x 32: resizing it back lands on many source values exactly
    means, scales = (127.5, 100.0, 0.0), (1.0, 0.5, 1.0)
    for (ho, wo) in ((16, 16), (24, 48)):
        fr, img = capi.frame_desc(1, 48, 32, capi.IMG_BGR), capi.image_desc(1, ho, wo, capi.IMG_BGR, means, scales)
        ref = image_to_tensor_ref(image_resize_ref(big, ho, wo), BGR, means, scales)
        for cs_ in (1.0, 0.5, 2.0):
            assert np.array_equal(gpu_ctx.frame_to_tensor(fr, img, big, cs_), plref.calib_f32_to_i8(ref, cs_))


def test_refusals_return_a_status(gpu_ctx, pkg):
    capi = pkg.capi
    z = np.zeros((1, 720, 640), np.uint8)
    with pytest.raises(capi.PlhipError):  # odd NV height
        gpu_ctx.image_convert(capi.frame_desc(1, 479, 640, capi.IMG_NV12), z)
    with pytest.raises(capi.PlhipError):  # odd NV width
        gpu_ctx.frame_to_tensor(capi.frame_desc(1, 480, 639, capi.IMG_NV21), capi.image_desc(1, 224, 224, capi.IMG_BGR, MEANS, SCALES), z)
    for dst in (capi.IMG_RGB, capi.IMG_RGBA, capi.IMG_GRAY):  # RGB-ordered destinations are not pinned by the reference
        with pytest.raises(capi.PlhipError):
            gpu_ctx.image_convert(capi.frame_desc(1, 480, 640, capi.IMG_NV12), z, dst)
    with pytest.raises(capi.PlhipError):  # an interleaved source has nothing to convert
        gpu_ctx.image_convert(capi.frame_desc(1, 240, 640, capi.IMG_BGR), z)
    for (h, w) in ((1, 8), (8, 1)):  # src < 2
        with pytest.raises(capi.PlhipError):
            gpu_ctx.image_resize(capi.frame_desc(1, h, w, capi.IMG_GRAY), np.zeros((1, h, w, 1), np.uint8), 4, 4)
    with pytest.raises(capi.PlhipError):  # the image's format must be BGR for an NV frame
        gpu_ctx.frame_to_tensor(capi.frame_desc(1, 480, 640, capi.IMG_NV12), capi.image_desc(1, 224, 224, capi.IMG_RGB, MEANS, SCALES), z)
    with gpu_ctx.scope() as s:
        d = s.put(z[:, :1])  # image_to_tensor keeps refusing NV (before it launches anything: d is never touched)
        for fmt in (capi.IMG_NV12, capi.IMG_NV21):
            nv_img = capi.image_desc(1, 480, 640, fmt, MEANS, SCALES)
            assert gpu_ctx.L.plhip_image_to_tensor_f32(gpu_ctx.h, ctypes.byref(nv_img), d, d) == -1
            assert gpu_ctx.L.plhip_image_to_tensor_i8(gpu_ctx.h, ctypes.byref(nv_img), d, d, 0.01) == -1
    gpu_ctx.sync()


def _run(lite, wl, net, batch, feed, fuse, image=None, frame=None, extra=()):
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, batch, fuse=fuse, image=image, frame=frame)
        plan = p.graph_plan()
        assert p.graph_lower() == [out]
        p.set_input(net["input"], feed)
        p.run()
        got = {out: p.get_var(out, np.float32)}
        for name, dt in extra:
            got[name] = p.get_var(name, dt)
        names = p.kernel_names()
        timed = [p.time_instruction(i, 2)[2] for i in range(1, 3)]
        return got, plan, names, timed
    finally:
        p.close()


@pytest.mark.parametrize("which", ["mobilenet_v1", "resnet50"])
def test_whole_program_nv12_frames_equal_image_feed(pkg, which):
    """Batch 2, fused and unfused, fed 480 x 640 NV12 frames, then (a second program on the same context, whose cached tables
    must follow) 720 x 1280 ones: every surviving variable equals the program fed the restated uint8 image through FeedImage."""
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    net = {"mobilenet_v1": wl.mobilenet_v1_net, "resnet50": wl.resnet50_net}[which]()
    c, h, w = net["input_shape"]
    batch = 2
    rng = np.random.default_rng(91)
    image = dict(format=BGR, means=MEANS, scales=SCALES)
    for (sh, sw) in ((480, 640), (720, 1280)):
        src = _nv_frame(rng, batch, sh, sw)
        small = image_resize_ref(nv_to_bgr_ref(src, False), h, w)
        frame = dict(h=sh, w=sw, format=NV12, means=MEANS, scales=SCALES)
        for fuse in (True, False):
            want, _, _, _ = _run(lite, wl, net, batch, small, fuse, image=image)
            extra = () if fuse else (("image/bgr", np.uint8), ("image/image", np.uint8), ("image/tensor", np.float32))
            got, plan, names, timed = _run(lite, wl, net, batch, src, fuse, frame=frame, extra=extra)
            (out,) = want.keys()
            assert np.array_equal(_bits(got[out]), _bits(want[out])), (which, sh, sw, fuse, int((got[out] != want[out]).sum()))
            if fuse:
                assert plan[1].startswith("image_resize/int8 in=image/target_trans out=image/precision_trans src=NV12 %dx%d->" % (sh, sw))
                assert any("image_resize:" in k and "nv12_image_resize_to_tensor_int8_hip" in k for k in names), names[:3]
                assert timed[0] == "nv12_image_resize_to_tensor_int8_hip"
            else:
                assert np.array_equal(got["image/bgr"], nv_to_bgr_ref(src, False))
                assert np.array_equal(got["image/image"], small)
                assert np.array_equal(_bits(got["image/tensor"]), _bits(image_to_tensor_ref(small, BGR, MEANS, SCALES)))
                assert any("image_convert:" in k and "nv12_to_bgr_u8_hip" in k for k in names), names[:4]
                assert any("image_resize:" in k and k.endswith("image_resize_u8_hip") for k in names), names[:4]
                assert timed == ["nv12_to_bgr_u8_hip", "image_resize_u8_hip"]


def test_program_bgr_frame_feed(pkg):
    """An interleaved 256 x 256 BGR frame into MobileNetV1, fused: image_resize/int8 from the BGR frame, equal to the image feed."""
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    net = wl.mobilenet_v1_net()
    c, h, w = net["input_shape"]
    rng = np.random.default_rng(92)
    src = rng.integers(0, 256, (2, 256, 256, 3)).astype(np.uint8)
    small = image_resize_ref(src, h, w)
    want, _, _, _ = _run(lite, wl, net, 2, small, True, image=dict(format=BGR, means=MEANS, scales=SCALES))
    got, plan, names, timed = _run(lite, wl, net, 2, src, True, frame=dict(h=256, w=256, format=BGR, means=MEANS, scales=SCALES))
    (k,) = want.keys()
    assert np.array_equal(_bits(got[k]), _bits(want[k]))
    assert " src=BGR 256x256->224x224 scale=" in plan[1] and timed[0] == "image_resize_to_tensor_int8_hip"
