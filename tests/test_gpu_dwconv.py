"""GPU: fusion G, depthwise 3x3 [int8_out] -> 1x1 conv with the conv's graph tail in one launch (plhip_dw_conv1x1_fused_int8),
against the oracle's two-stage computation (depthwise int8_out, then the 1x1 conv and its tail) and against the two launches
it replaces; and the MobileNetV2 / MobileNetV1-192 programs lowered with GraphBuilder::set_fuse_dwconv(true)."""
import ctypes
import importlib

import numpy as np
import pytest

from oracle import graph_oracle

pytestmark = pytest.mark.gpu

FUSED = "conv_depthwise_3x3_conv1x1_fused_int8_hip"

# MobileNetV2-224's 17 blocks: (C, input plane, stride, M, tail) — tail "res" = residual add + calib copy (the fp32 sum
# dropped or kept), "calib" = calib copy of the fp32 output, "i8" = plain int8_out project conv (b1, b17)
V2_BLOCKS = [
    (32, 112, 1, 16, "i8"), (96, 112, 2, 24, "calib"), (144, 56, 1, 24, "res"), (144, 56, 2, 32, "calib"),
    (192, 28, 1, 32, "res"), (192, 28, 1, 32, "res"), (192, 28, 2, 64, "calib"), (384, 14, 1, 64, "res"),
    (384, 14, 1, 64, "res"), (384, 14, 1, 64, "res"), (384, 14, 1, 96, "calib"), (576, 14, 1, 96, "res"),
    (576, 14, 1, 96, "res"), (576, 14, 2, 160, "calib"), (960, 7, 1, 160, "res"), (960, 7, 1, 160, "res"),
    (960, 7, 1, 320, "i8"),
]


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


def _case(ctx, capi, plref, rng, n, c, h, w, stride, pad, m, tail, dw_act=2, pw_act=0, dw_alpha=6.0, pw_alpha=6.0,
          residual_relu=False, want_y=True):
    """One pair through the fused entry point, checked against the oracle and against the two launches it replaces."""
    x = rng.integers(-127, 128, (n, c, h, w)).astype(np.int8)
    w_dw = rng.integers(-127, 128, (c, 1, 3, 3)).astype(np.int8)
    w_pw = rng.integers(-127, 128, (m, c, 1, 1)).astype(np.int8)
    b_dw = rng.uniform(-1, 1, c).astype(np.float32)
    b_pw = rng.uniform(-1, 1, m).astype(np.float32)
    ws_dw = ((1 + np.arange(c) % 7) / 127.0 / 4.0).astype(np.float32)
    ws_pw = ((1 + np.arange(m) % 5) / 127.0 / 4.0).astype(np.float32)
    int8_out = tail == "i8"
    in_s, mid_s = 1 / 127.0, (9 / 127.0 if dw_act != 2 else dw_alpha / 127.0)
    out_s = c / 127.0 / 8 if pw_act != 2 else pw_alpha / 127.0
    sd = plref.shape(n, c, h, w, c, 3, 3, pad, (stride, stride), (1, 1), c)
    oh, ow = plref.out_dims(sd)
    s1, b1, a1 = plref.fold_scales(1, in_s, ws_dw, mid_s, b_dw, c, dw_act, dw_alpha)
    d_ref, _ = plref.conv2d(sd, x, w_dw, b_dw, in_s, ws_dw, mid_s, dw_act, dw_alpha, True)
    sp = plref.shape(n, c, oh, ow, m, 1, 1, (0, 0, 0, 0), (1, 1), (1, 1), 1)
    y_ref, acc_ref = plref.conv2d(sp, d_ref, w_pw, b_pw, mid_s, ws_pw, out_s, pw_act, pw_alpha, int8_out)
    s2, b2, a2 = plref.fold_scales(int(int8_out), mid_s, ws_pw, out_s, b_pw, m, pw_act, pw_alpha)
    d_dw = capi.conv_desc(n, c, h, w, c, 3, 3, pad, (stride, stride), (1, 1), c, dw_act, a1)
    has_tail = tail in ("res", "calib")
    kind = capi.OUT_I8 if int8_out else capi.OUT_F32
    assert ctx.L.plhip_dw_conv1x1_fused_supported(ctypes.byref(d_dw), m, kind, int(has_tail)) == 1, (n, c, h, w, stride, pad, m)
    acc, _ = ctx.dw_conv1x1_fused(d_dw, x, w_dw, s1, b1, w_pw, None, None, pw_act, a2, capi.OUT_I32)
    assert np.array_equal(acc, acc_ref), "fused int32 accumulators differ (%d of %d)" % ((acc != acc_ref).sum(), acc.size)
    if int8_out:
        y, _ = ctx.dw_conv1x1_fused(d_dw, x, w_dw, s1, b1, w_pw, s2, b2, pw_act, a2, capi.OUT_I8)
        assert np.array_equal(y, y_ref), "fused int8 output differs (%d values)" % (y != y_ref).sum()
        return
    res = rng.standard_normal(y_ref.shape).astype(np.float32) * np.float32(y_ref.std()) if tail == "res" else None
    z = plref.elementwise_add(y_ref, res, residual_relu) if res is not None else y_ref
    cs = float(np.abs(z).max() / 100.0) if has_tail else None
    yf, yq = ctx.dw_conv1x1_fused(d_dw, x, w_dw, s1, b1, w_pw, s2, b2, pw_act, a2, capi.OUT_F32, residual=res,
                                  residual_relu=int(residual_relu), calib_scale=cs, want_y=want_y)
    # the two launches the fused one replaces, on the device: bit for bit
    mid = ctx.conv2d(d_dw, x, w_dw, s1, b1, capi.OUT_I8, depthwise=True)
    assert np.array_equal(mid, d_ref)
    d_pw = capi.conv_desc(n, c, oh, ow, m, 1, 1, act=pw_act, alpha=a2)
    if has_tail:
        tf, tq = ctx.conv2d_fused(d_pw, mid, w_pw, s2, b2, res, int(residual_relu), cs, want_y)
    else:
        tf, tq = ctx.conv2d(d_pw, mid, w_pw, s2, b2, capi.OUT_F32), None
    if want_y:
        np.testing.assert_allclose(yf, z, rtol=1e-5, atol=1e-6)
        assert np.array_equal(yf.view(np.int32), tf.view(np.int32)), "fp32 output differs from the two launches"
    else:
        assert yf is None
    if has_tail:
        assert np.array_equal(yq, tq), "calib copy differs from the two launches"
        assert np.array_equal(yq, plref.calib_f32_to_i8(z, cs)), "calib copy differs from the oracle"


def test_mobilenet_v2_block_shapes(gpu_ctx, pkg, plref):
    """The 17 block pairs of MobileNetV2-224 at n = 2 with their real tails (relu6 depthwise, linear project conv); every
    other residual block drops the fp32 sum (y == NULL, calib copy only)."""
    rng = np.random.default_rng(900)
    for i, (c, hw, s, m, tail) in enumerate(V2_BLOCKS):
        _case(gpu_ctx, pkg.capi, plref, rng, 2, c, hw, hw, s, (1, 1, 1, 1), m, tail, want_y=not (tail == "res" and i % 2 == 0))


def test_off_v2_shapes(gpu_ctx, pkg, plref):
    capi = pkg.capi
    rng = np.random.default_rng(901)
    cases = [
        # n, c, h, w, stride, pad (t, b, l, r), m, tail, dw_act, pw_act, residual_relu
        (2, 16, 9, 13, 2, (0, 1, 1, 0), 8, "calib", 1, 0, False),      # odd plane, asymmetric pads, M = 8, C = 16
        (3, 16, 10, 10, 1, (1, 1, 1, 1), 40, "i8", 4, 1, False),       # C = 16, leaky depthwise, relu 1x1
        (1, 1024, 7, 7, 1, (1, 1, 1, 1), 1024, "res", 1, 1, True),     # C = M = 1024, residual relu
        (2, 256, 24, 24, 1, (1, 1, 1, 1), 256, "i8", 1, 1, False),     # MobileNetV1-192 pairs
        (2, 128, 48, 48, 2, (1, 1, 1, 1), 256, "i8", 1, 1, False),
        (2, 512, 12, 12, 2, (1, 1, 1, 1), 1024, "i8", 1, 1, False),
        (2, 64, 20, 20, 1, (0, 0, 0, 0), 72, "res", 4, 4, True),       # leaky both, no padding, residual relu
        (2, 48, 15, 11, 1, (1, 0, 0, 1), 24, "i8", 2, 2, False),       # relu6 on both, int8 out
        (2, 32, 14, 14, 1, (1, 1, 1, 1), 64, "none", 0, 2, False),     # fp32 output, no tail, no depthwise activation
    ]
    for (n, c, h, w, s, pad, m, tail, da, pa, rr) in cases:
        _case(gpu_ctx, capi, plref, rng, n, c, h, w, s, pad, m, tail, dw_act=da, pw_act=pa, residual_relu=rr)


def test_batch_128_tile_regimes(gpu_ctx, pkg, plref):
    """Real grid sizes: a large plane with the residual + calib tail, a 7 x 7 plane with the widest K."""
    rng = np.random.default_rng(902)
    _case(gpu_ctx, pkg.capi, plref, rng, 128, 144, 56, 56, 1, (1, 1, 1, 1), 24, "res")
    _case(gpu_ctx, pkg.capi, plref, rng, 128, 960, 7, 7, 1, (1, 1, 1, 1), 160, "res", want_y=False)


def test_unsupported_shapes_write_nothing(gpu_ctx, pkg):
    capi = pkg.capi
    n, c, h = 2, 32, 8
    for (d, m, out, tail) in [
        (capi.conv_desc(n, c, h, h, c, 5, 5, (2, 2, 2, 2), (1, 1), (1, 1), c), 16, capi.OUT_F32, False),   # 5x5
        (capi.conv_desc(n, c, h, h, c, 3, 3, (2, 2, 2, 2), (1, 1), (2, 2), c), 16, capi.OUT_F32, False),   # dilation 2
        (capi.conv_desc(n, 24, h, h, 24, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 24), 16, capi.OUT_F32, False),  # C = 24
        (capi.conv_desc(n, c, h, h, c, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), c), 33, capi.OUT_F32, False),   # M = 33
        (capi.conv_desc(n, c, h, h, c, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), c), 16, capi.OUT_I8, True),     # tail with int8 out
    ]:
        assert gpu_ctx.L.plhip_dw_conv1x1_fused_supported(ctypes.byref(d), m, out, int(tail)) == 0
        oh, ow = capi.out_hw(d)
        cnt = n * m * oh * ow
        sentinel = np.full(cnt * 4, 0x5a, np.uint8)
        with gpu_ctx.scope() as s:
            dy, dq = s.put(sentinel), s.put(sentinel[:cnt])
            kx = s.alloc(n * d.cin * h * h + 64)
            kw = s.alloc(d.cin * 25 + 64)
            ks = s.alloc(4096 * 4)
            kp = s.alloc(1 << 16)
            dr = s.alloc(cnt * 4) if tail else ctypes.c_void_p()
            st = gpu_ctx.L.plhip_dw_conv1x1_fused_int8(gpu_ctx.h, ctypes.byref(d), kx, kw, ks, None, m, kp, ks, None, 0, 0.0, dy, out,
                                                       dr, 0, dq if tail else None, 1.0)
            assert st == -3, st
            gpu_ctx.sync()
            assert np.array_equal(gpu_ctx.to_host(dy, sentinel.shape, np.uint8), sentinel)
            assert np.array_equal(gpu_ctx.to_host(dq, (cnt,), np.uint8), sentinel[:cnt])


def _run_graph(lite, wl, net, img):
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, img.shape[0], fuse=True, fuse_dwconv=True)
        assert p.graph_lower() == [out]
        p.set_input(net["input"], img)
        p.run()
        p.run(skip_io_copy=False)  # second launch: ReInitWhenNeeded no-op paths
        return p, out
    except Exception:
        p.close()
        raise


def _compare_materialised(p, ref, out):
    """Every variable the fused program still materialises against the oracle: int8 bit for bit, fp32 within 1e-5, prob 1e-4."""
    n_i8 = n_f32 = 0
    for name, want in ref.items():
        try:
            got = p.get_var(name, want.dtype)
        except Exception:  # noqa: BLE001  (a variable the fused program does not materialise)
            continue
        assert got.shape == want.shape, name
        if want.dtype == np.int8:
            assert np.array_equal(got, want), "%s: %d of %d int8 values differ" % (name, (got != want).sum(), want.size)
            n_i8 += 1
        else:
            np.testing.assert_allclose(got, want, rtol=1e-4 if name == out else 1e-5, atol=1e-7 if name == out else 1e-5,
                                       err_msg=name)
            n_f32 += 1
    return n_i8, n_f32


def test_mobilenet_v2_graph_with_fusion_g(lite, wl, plref):
    net = wl.mobilenet_v2_net()
    img = np.random.default_rng(903).uniform(-1, 1, (3, 3, 224, 224)).astype(np.float32)
    ref = graph_oracle.forward(plref, net, img)
    p, out = _run_graph(lite, wl, net, img)
    try:
        names = p.kernel_names()
        assert sum(FUSED in n for n in names) == 17, names
        n_i8, n_f32 = _compare_materialised(p, ref, out[:-len("/host")])
        assert n_i8 >= 30 and n_f32 >= 5 and "prob" in ref
    finally:
        p.close()


def _big_batch_check(lite, wl, plref, net, B, seed, mid):
    """The fused program at the benchmark batch: the first two images reproduce the batch-2 run bit for bit, and one image
    from the middle of the batch equals the oracle."""
    rng = np.random.default_rng(seed)
    c, h, w = net["input_shape"]
    img = rng.uniform(-1, 1, (B, c, h, w)).astype(np.float32)
    ref_mid = graph_oracle.forward(plref, net, img[mid:mid + 1], via_gemm=True)
    small, out = _run_graph(lite, wl, net, img[:2])
    try:
        big, out_b = _run_graph(lite, wl, net, img)
        try:
            assert out == out_b
            assert sum(FUSED in n for n in big.kernel_names()) == 17
            n_i8 = n_f32 = 0
            for name, want in ref_mid.items():
                try:
                    s_ = small.get_var(name, want.dtype)
                except Exception:  # noqa: BLE001  (a variable the fused program does not materialise)
                    continue
                g_ = big.get_var(name, want.dtype, max_bytes=int(want.nbytes) * B + 64)
                assert g_.shape[0] == B and s_.shape[0] == 2, name
                if want.dtype == np.int8:
                    assert np.array_equal(g_[:2], s_), "%s: batch-%d prefix differs from the batch-2 run" % (name, B)
                    assert np.array_equal(g_[mid:mid + 1], want), "%s: image %d differs from the oracle" % (name, mid)
                    n_i8 += 1
                else:
                    np.testing.assert_array_equal(g_[:2], s_, err_msg=name)
                    np.testing.assert_allclose(g_[mid:mid + 1], want, rtol=1e-4 if name == out else 1e-5, atol=1e-5, err_msg=name)
                    n_f32 += 1
            return n_i8, n_f32
        finally:
            big.close()
    finally:
        small.close()


def test_mobilenet_v2_graph_with_fusion_g_at_batch_1024(lite, wl, plref):
    n_i8, n_f32 = _big_batch_check(lite, wl, plref, wl.mobilenet_v2_net(), 1024, 904, mid=611)
    assert n_i8 >= 30 and n_f32 >= 2


def test_mobilenet_v1_192_graph_with_fusion_g(lite, wl, plref):
    net = wl.mobilenet_v1_net(res=192)
    img = np.random.default_rng(905).uniform(-1, 1, (2, 3, 192, 192)).astype(np.float32)
    ref = graph_oracle.forward(plref, net, img)
    p, out = _run_graph(lite, wl, net, img)
    try:
        assert sum(FUSED in n for n in p.kernel_names()) == 13
        n_i8, n_f32 = _compare_materialised(p, ref, out[:-len("/host")])
        assert n_i8 >= 10 and n_f32 >= 1
    finally:
        p.close()


def test_fusion_g_falls_back_inside_the_kernel_object(lite, wl, plref, pkg):
    """MobileNetV2 lowered with G (17 one-launch instructions); then the fused path is switched off (diagnostics knob
    DWCONV_FUSED = 0: the predicate refuses every shape) and the feed resized, so every fused instruction re-initialises and
    runs its two instructions inside the kernel object (depthwise into a private tensor, then plhip_conv2d_int8_fused with
    the residual / calib / dropped-fp32 tail, or plhip_conv2d_int8 for the int8_out pairs) and must still equal the oracle;
    with the knob back on the first result is reproduced."""
    L = pkg.capi.load()
    net = wl.mobilenet_v2_net()
    rng = np.random.default_rng(906)
    img2 = rng.uniform(-1, 1, (2, 3, 224, 224)).astype(np.float32)
    img3 = rng.uniform(-1, 1, (3, 3, 224, 224)).astype(np.float32)
    ref3 = graph_oracle.forward(plref, net, img3)
    p, out = _run_graph(lite, wl, net, img2)
    dev_out = out[:-len("/host")]
    try:
        assert sum(FUSED in n for n in p.kernel_names()) == 17
        first = p.get_var(dev_out, np.float32)
        assert L.plhip_debug_set(b"DWCONV_FUSED", 0) == 0
        p.add_feed(net["input"], img3.shape, lite.PREC_FLOAT)
        p.set_input(net["input"], img3)
        p.run()
        names = p.kernel_names()
        assert sum("conv_depthwise_int8_hip+conv1x1_tail_gemm_int8_hip" in n for n in names) == 17, names
        assert not any(FUSED in n for n in names)
        n_i8, n_f32 = _compare_materialised(p, ref3, dev_out)
        assert n_i8 >= 30 and n_f32 >= 5
        assert L.plhip_debug_set(b"DWCONV_FUSED", 1) == 0
        p.add_feed(net["input"], img2.shape, lite.PREC_FLOAT)
        p.set_input(net["input"], img2)
        p.run()
        assert sum(FUSED in n for n in p.kernel_names()) == 17
        assert np.array_equal(p.get_var(dev_out, np.float32), first)
    finally:
        L.plhip_debug_set(b"DWCONV_FUSED", 1)
        p.close()
