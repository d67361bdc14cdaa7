"""uint8 image input on the MI355X, all bit-exact: plhip_image_to_tensor_f32 / _i8 against the numpy restatement of image2tensor.cc
(+ the oracle's calib), the fused uint8 stem (conv_stem_u8in.hip) against restatement -> calib -> the oracle's conv, and whole
programs fed one uint8 image batch against the same program fed the restated fp32 tensor through the existing fp32 path."""
import ctypes
import importlib

import numpy as np
import pytest

from test_image_feed_host import BGR, BGRA, GRAY, MEANS, PIXEL_BYTES, RGB, RGBA, SCALES, image_to_tensor_ref

pytestmark = pytest.mark.gpu

FORMATS = (RGBA, BGRA, RGB, BGR, GRAY)


def _image(rng, n, h, w, fmt):
    return rng.integers(0, 256, (n, h, w, PIXEL_BYTES[fmt])).astype(np.uint8)


def test_image_to_tensor_kernels(gpu_ctx, pkg, plref):
    """Every format, n in {1, 3}, w in {1, 7, 223, 224}: the vector path (h * w % 16 == 0) and the scalar one."""
    capi = pkg.capi
    rng = np.random.default_rng(2024)
    calib_scale = 1.0 / 127 * 1.1
    for fmt in FORMATS:
        for n in (1, 3):
            for (h, w) in ((5, 1), (3, 7), (4, 223), (6, 224), (224, 224)):
                if (h, w) == (224, 224) and n == 3 and fmt not in (BGR, GRAY):
                    continue
                src = _image(rng, n, h, w, fmt)
                img = capi.image_desc(n, h, w, fmt, MEANS, SCALES)
                ref = image_to_tensor_ref(src, fmt, MEANS, SCALES)
                y = gpu_ctx.image_to_tensor(img, src)
                assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), ref.view(np.uint32)), (fmt, n, h, w)
                q = gpu_ctx.image_to_tensor(img, src, calib_scale)
                assert np.array_equal(q, plref.calib_f32_to_i8(ref, calib_scale)), (fmt, n, h, w)


def test_image_to_tensor_rounding_ties(gpu_ctx, pkg, plref):
    """Means / scales chosen so that many normalised values land on the calib's rounding ties and past its saturation bound."""
    capi = pkg.capi
    src = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3).copy()
    src[..., 1] = src[..., 1][:, ::-1]
    means, scales = (127.5, 100.0, 0.0), (1.0, 0.5, 1.0)
    img = capi.image_desc(1, 16, 16, capi.IMG_BGR, means, scales)
    ref = image_to_tensor_ref(src, BGR, means, scales)
    for cs_ in (1.0, 0.5, 2.0):
        assert np.array_equal(gpu_ctx.image_to_tensor(img, src, cs_), plref.calib_f32_to_i8(ref, cs_))


def test_fused_uint8_stem(gpu_ctx, pkg, plref):
    """plhip_conv2d_image_int8 against restatement -> calib -> the oracle's conv: I32 / I8 / F32 outputs, the four activations,
    top padding 0 and 1, two column tiles (w > 256), Cout tails, GRAY with cin 1, the 4-byte formats."""
    capi = pkg.capi
    rng = np.random.default_rng(355)
    cnt = 0
    for (n, fmt, h, w, cout, pads) in [(2, BGR, 224, 224, 32, (1, 1, 1, 1)), (1, RGB, 16, 16, 33, (1, 1, 1, 1)),
                                       (3, GRAY, 18, 32, 8, (1, 1, 1, 1)), (1, BGRA, 21, 264, 64, (1, 1, 1, 1)),
                                       (2, RGBA, 10, 8, 40, (0, 1, 1, 0)), (1, BGR, 66, 520, 40, (1, 0, 1, 1))]:
        cin = 1 if fmt == GRAY else 3
        act = (1, 0, 2, 4)[cnt % 4]
        alpha = 6.0 if act == 2 else 0.2
        calib_scale = float(np.float32(1.0 / 127 * (1 + cnt % 3)))
        src = _image(rng, n, h, w, fmt)
        img = capi.image_desc(n, h, w, fmt, MEANS, SCALES)
        x = plref.calib_f32_to_i8(image_to_tensor_ref(src, fmt, MEANS, SCALES), calib_scale)
        wt = rng.integers(-127, 128, (cout, cin, 3, 3)).astype(np.int8)
        bias = rng.uniform(-1, 1, cout).astype(np.float32) if cnt % 2 == 0 else None
        w_scale = ((1 + np.arange(cout) % 7) / 127.0 / 4.0).astype(np.float32)
        out_scale = cin * 9 / 127.0 if act != 2 else alpha / 127.0
        s = plref.shape(n, cin, h, w, cout, 3, 3, pads, (2, 2), (1, 1), 1)
        acc_ref = plref.conv2d_acc(s, x, wt)
        d = capi.conv_desc(n, cin, h, w, cout, 3, 3, pads, (2, 2), (1, 1), 1, act, alpha)
        assert gpu_ctx.L.plhip_conv2d_image_supported(ctypes.byref(d), ctypes.byref(img)) == 1
        acc = gpu_ctx.conv2d_image(d, img, src, calib_scale, wt, None, None, capi.OUT_I32)
        assert np.array_equal(acc, acc_ref), "int32 accumulators differ (%d of %d)" % ((acc != acc_ref).sum(), acc.size)
        for int8_out, kind in ((0, capi.OUT_F32), (1, capi.OUT_I8)):
            sc, bi, al = plref.fold_scales(int8_out, calib_scale, w_scale, out_scale, bias, cout, act, alpha)
            d.act_alpha = al
            y_ref = plref.epilogue(acc_ref, sc, bi, act, al, bool(int8_out))
            y = gpu_ctx.conv2d_image(d, img, src, calib_scale, wt, sc, bi if bias is not None else None, kind)
            # the same instruction run as separate kernels: image_to_tensor_i8 then the plain conv
            y2 = gpu_ctx.conv2d(d, gpu_ctx.image_to_tensor(img, src, calib_scale), wt, sc, bi if bias is not None else None, kind)
            assert np.array_equal(y.view(np.uint8), y2.view(np.uint8)), "fused stem differs from the two kernels"
            if int8_out:
                assert np.array_equal(y, y_ref), "int8 output differs"
            else:
                np.testing.assert_allclose(y, y_ref, rtol=1e-5, atol=1e-6)
        cnt += 1
    # outside the envelope: the call refuses and launches nothing
    d = capi.conv_desc(1, 3, 30, 30, 8, 3, 3, (1, 1, 1, 1), (2, 2))
    with pytest.raises(capi.PlhipError):
        gpu_ctx.conv2d_image(d, capi.image_desc(1, 30, 30, capi.IMG_BGR, MEANS, SCALES), np.zeros((1, 30, 30, 3), np.uint8), 0.01,
                             np.zeros((8, 3, 3, 3), np.int8), None, None, capi.OUT_I32)


def _run_program(lite, wl, net, batch, feed, image):
    """Lower `net` with the default fusions, feed it, run it with the io_copy inside (skip_io_copy=False); (output, plan, kernels)."""
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, batch, image=image)
        plan = p.graph_plan()
        assert p.graph_lower() == [out]
        p.set_input(net["input"], feed)
        p.run()
        y = p.get_var(out, np.float32)
        return y, plan, p.kernel_names()
    finally:
        p.close()


@pytest.mark.parametrize("which,batch", [("mobilenet_v1", 2), ("mobilenet_v1", 128), ("mobilenet_v2", 2), ("resnet50", 2)])
def test_whole_program_uint8_feed_equals_fp32_feed(pkg, which, batch):
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    net = {"mobilenet_v1": wl.mobilenet_v1_net, "mobilenet_v2": wl.mobilenet_v2_net, "resnet50": wl.resnet50_net}[which]()
    c, h, w = net["input_shape"]
    rng = np.random.default_rng(77 + batch)
    src = rng.integers(0, 256, (batch, h, w, 3)).astype(np.uint8)
    xf = image_to_tensor_ref(src, BGR, MEANS, SCALES)
    y_f32, _, _ = _run_program(lite, wl, net, batch, xf, None)
    y_img, plan, kernels = _run_program(lite, wl, net, batch, src, dict(format=BGR, means=MEANS, scales=SCALES))
    assert np.array_equal(y_img.view(np.uint32), y_f32.view(np.uint32)), "%d of %d outputs differ" % ((y_img != y_f32).sum(), y_img.size)
    if which == "resnet50":
        assert plan[1].startswith("image_to_tensor/int8 ")
        assert any("image_to_tensor_int8_hip" in k for k in kernels)
    else:
        assert " +image_in=image fmt=BGR " in plan[1]
        assert any("image_to_tensor_int8+" in k for k in kernels), kernels[:3]
