"""-m gpu: bilinear_interp / nearest_interp, arg_max and interp -> arg_max in one launch on the device (csrc/interp_ops.hip) through
the C ABI.  plhip_interp_f32 against interp_oracle (fp32 compared as uint32: the arithmetic is fully specified, and one ulp would
flip int8 ties and labels; int8 exactly) in bilinear's three modes and nearest's two, with and without the fp32 output, on both
item widths (quads and elements) and with every base off alignment by one element, and against the two device calls it replaces
(NaN and infinities included); plhip_arg_max_f32 with exact ties planted; plhip_interp_argmax_f32 against the oracle and against
the two device calls, on the LDS path and on the direct one; the refusals of all three; the kernel classes through
KernelFactory -> SetParam -> Launch."""
import ctypes as C
import importlib

import numpy as np
import pytest

import interp_oracle as I
import shuffle_oracle as S

pytestmark = pytest.mark.gpu
F32 = np.float32
SCALES = (4.0 / 127, 0.03125)  # test_gpu_concat_calib.py's: the networks' scale, and a power of two ((k + 0.5) * scale / scale is a tie exactly)
# (method, align_corners, align_mode)
MODES = [("bilinear", True, 1), ("bilinear", False, 0), ("bilinear", False, 1), ("nearest", True, 1), ("nearest", False, 1)]


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _inputs(rng, shape, scale, nonfinite=False):
    """randn * 2 (a real share beyond +-127 steps of either scale) with the ties (k + 0.5) * scale, k = 0 .. 127, in both signs
    (+-127.5 * scale among them), values far outside the range, denormals and +-0 planted; nonfinite: NaN (two payloads) and +-inf too."""
    x = (rng.standard_normal(shape) * 2).astype(F32)
    flat = x.reshape(-1)
    k = np.arange(0, 128, dtype=np.float64)
    ties = np.concatenate([(k + 0.5) * scale, -(k + 0.5) * scale]).astype(F32)   # +-0.5 .. +-127.5 steps
    edge = np.concatenate([np.array([0.0, -0.0, 127.5 * scale, -127.5 * scale, 1e30, -1e30, 3e38, -3e38, 1000.0, -1000.0, 1e-40, -1e-40], F32), ties])
    if nonfinite:
        edge = np.concatenate([np.array([np.nan, np.inf, -np.inf, np.nan], F32), edge])
    n = min(flat.size, edge.size)
    pos = rng.permutation(flat.size)[:n]
    flat[pos] = edge[:n]
    if nonfinite:
        flat.view(np.uint32)[pos[0]] = 0x7FC12345  # a NaN with a payload of its own
    return x


# (planes, in_h, in_w, out_h, out_w)
CASES = [(1, 1, 1, 1, 1), (3, 1, 1, 4, 5), (2, 2, 2, 2, 2), (6, 7, 5, 28, 20), (4, 8, 8, 15, 17), (2, 16, 16, 64, 64),
         (3, 9, 13, 4, 6), (1, 3, 3, 1, 7), (2, 33, 33, 129, 129)]


@pytest.mark.parametrize("planes,ih,iw,oh,ow", CASES)
def test_interp_equals_the_oracle_and_the_two_calls(gpu_ctx, planes, ih, iw, oh, ow):
    rng = np.random.default_rng(580 + planes + 3 * ih + 5 * iw + 7 * oh + 11 * ow)
    for scale in SCALES:
        x = _inputs(rng, (planes, ih, iw), scale)
        z = _inputs(rng, (planes, ih, iw), scale, nonfinite=True)
        for method, ac, am in MODES:
            want_f = I.interp(x, (oh, ow), method, ac, am)
            want_q = S.calib_i8(want_f, scale)
            assert want_f.shape == (planes, oh, ow) and want_f.dtype == F32
            if ac and (ih, iw, oh, ow) == (33, 33, 129, 129):
                # out = (in - 1) * 4 + 1 with aligned corners: every source pixel is copied exactly (f = l / 4, weights 1 and 0), so
                # the planted ties and the saturating values reach the quantiser
                assert np.array_equal(want_f[:, ::4, ::4], x)
                assert want_q.min() == -127 and want_q.max() == 127
            ab_f, _ = gpu_ctx.interp(z, (oh, ow), method, ac, am, mode="f32")      # the two calls the one launch replaces
            ab_q = gpu_ctx.calib_f32_to_i8(ab_f, scale)
            for mis in (0, 1):
                for mode in ("both", "i8"):
                    what = "interp %s %s ac %d am %d scale %g misalign %d %s" % ((planes, ih, iw, oh, ow), method, ac, am, scale, mis, mode)
                    yf, yq = gpu_ctx.interp(x, (oh, ow), method, ac, am, mode=mode, calib_scale=scale, misalign=mis)
                    assert yq.shape == want_q.shape and yq.dtype == np.int8, what
                    assert np.array_equal(yq, want_q), "%s: %d of %d int8 values differ from the oracle" % (what, (yq != want_q).sum(), want_q.size)
                    assert not (yq == -128).any(), what
                    if mode == "both":
                        bad = _bits(yf) != _bits(want_f)
                        assert not bad.any(), "%s: %d of %d fp32 values differ in their bits from the oracle" % (what, bad.sum(), bad.size)
                    else:
                        assert yf is None
                    zf, zq = gpu_ctx.interp(z, (oh, ow), method, ac, am, mode=mode, calib_scale=scale, misalign=mis)
                    assert zq.tobytes() == ab_q.tobytes(), "%s: %d int8 values differ from interp + calib on the device" % (what, (zq != ab_q).sum())
                    assert not (zq == -128).any(), what
                    if mode == "both":
                        assert zf.tobytes() == ab_f.tobytes(), what + ": fp32 differs between the aligned and the element path"


def test_interp_f32_alone_equals_the_oracle(gpu_ctx):
    rng = np.random.default_rng(581)
    x = _inputs(rng, (6, 7, 5), SCALES[0])
    for method, ac, am in MODES:
        for mis in (0, 1):
            yf, yq = gpu_ctx.interp(x, (28, 20), method, ac, am, mode="f32", misalign=mis)
            assert yq is None and np.array_equal(_bits(yf), _bits(I.interp(x, (28, 20), method, ac, am))), (method, ac, am, mis)


def _with_ties(rng, x, axis):
    """Two channels of x along `axis` set to the maximum over the axis at about half of the positions: exact ties that are maximal."""
    c = x.shape[axis]
    if c < 2:
        return x
    a, b = sorted(rng.choice(c, 2, replace=False))
    m = x.max(axis=axis, keepdims=True)
    mask = rng.random(m.shape) < 0.5
    x = np.moveaxis(x, axis, 0)
    mm, mk = np.moveaxis(m, axis, 0)[0], np.moveaxis(mask, axis, 0)[0]
    x[a] = np.where(mk, mm, x[a])
    x[b] = np.where(mk, mm, x[b])
    return np.ascontiguousarray(np.moveaxis(x, 0, axis))


def _tied(x, axis):
    """How many positions have their maximum along `axis` more than once."""
    return int(((x == x.max(axis=axis, keepdims=True)).sum(axis=axis) > 1).sum())


@pytest.mark.parametrize("shape", [(2, 19, 35), (1, 1, 7), (3, 5, 1), (2, 300, 4)])
def test_arg_max_takes_the_largest_index_among_ties(gpu_ctx, shape):
    rng = np.random.default_rng(582 + sum(shape))
    x = _with_ties(rng, rng.standard_normal(shape).astype(F32), 1)
    if shape[1] > 1:
        assert _tied(x, 1) > 0
    for dtype, np_t in ((-1, np.int64), (3, np.int64), (2, np.int32)):
        for keepdims in (False, True):
            want = I.arg_max(x, 1, dtype, keepdims)
            for mis in (0, 1):
                got = gpu_ctx.arg_max(x, 1, dtype, keepdims, misalign=mis)
                assert got.dtype == np_t and got.shape == want.shape and np.array_equal(got, want), (shape, dtype, keepdims, mis)
    # the larger index, not the first: numpy's own argmax takes the first and differs wherever there is a tie
    if shape[1] > 1:
        assert (gpu_ctx.arg_max(x, 1) != np.argmax(x, axis=1)).sum() == _tied(x, 1)
    # another axis: outer 1 / inner large, and the last axis (inner 1)
    for axis in (0, 2):
        assert np.array_equal(gpu_ctx.arg_max(x, axis), I.arg_max(x, axis)), (shape, axis)


# (in_h, in_w, out_h, out_w)
HEADS = [(8, 8, 32, 32), (5, 7, 17, 25), (33, 33, 129, 129)]
LDS_BYTES = 65536


@pytest.mark.parametrize("ih,iw,oh,ow", HEADS)
@pytest.mark.parametrize("c", [1, 2, 19, 21, 480])
def test_interp_argmax_equals_the_oracle_and_the_two_calls(gpu_ctx, c, ih, iw, oh, ow):
    """c = 480: the smallest source window of a tile here is the whole 5 x 7 source, 480 * 35 * 4 bytes > 64 KB: the direct path at every
    shape.  21 classes are staged in LDS at every shape (the largest window, 33 x 33 -> 129 x 129 by 4, is at most 11 x 11)."""
    assert 480 * 5 * 7 * 4 > LDS_BYTES > 21 * 11 * 11 * 4
    n = 2 if c < 100 else 1
    rng = np.random.default_rng(583 + c + ih + ow)
    x = _with_ties(rng, rng.standard_normal((n, c, ih, iw)).astype(F32), 1)
    for k, (method, ac, am) in enumerate(MODES):
        up = I.interp(x, (oh, ow), method, ac, am)
        if c > 1:
            assert _tied(up, 1) > 0   # the duplicated channels resample to the same bits: ties survive the interpolation
        dev_up, _ = gpu_ctx.interp(x, (oh, ow), method, ac, am, mode="f32")
        for dtype in (-1, 2):
            want = I.arg_max(up, 1, dtype)
            two = gpu_ctx.arg_max(dev_up, 1, dtype)
            for mis in (0, 1):
                got = gpu_ctx.interp_argmax(x, (oh, ow), method, ac, am, dtype=dtype, misalign=mis)
                what = "interp_argmax c %d %s %s ac %d am %d dtype %d misalign %d" % (c, (ih, iw, oh, ow), method, ac, am, dtype, mis)
                assert got.dtype == want.dtype and got.shape == (n, oh, ow), what
                assert np.array_equal(got, want), "%s: %d labels differ from the oracle" % (what, (got != want).sum())
                assert np.array_equal(got, two), "%s: %d labels differ from interp + arg_max on the device" % (what, (got != two).sum())


def test_nan_logits_give_a_label_in_range_and_the_two_forms_agree(gpu_ctx):
    rng = np.random.default_rng(584)
    n, c, ih, iw, oh, ow = 2, 19, 8, 8, 32, 32
    x = rng.standard_normal((n, c, ih, iw)).astype(F32)
    flat = x.reshape(-1)
    flat[rng.permutation(flat.size)[:200]] = np.nan
    x[0, :, 3, 3] = np.nan      # every channel of a pixel
    x[1, 0, :, :] = np.nan      # channel 0 everywhere
    flat[rng.permutation(flat.size)[:20]] = np.inf
    for method, ac, am in MODES:
        dev_up, _ = gpu_ctx.interp(x, (oh, ow), method, ac, am, mode="f32")
        assert np.isnan(dev_up).any()
        two = gpu_ctx.arg_max(dev_up, 1)
        got = gpu_ctx.interp_argmax(x, (oh, ow), method, ac, am)
        assert got.min() >= 0 and got.max() < c and np.array_equal(got, two), (method, ac, am)
    lab = gpu_ctx.arg_max(np.full((2, 5, 9), np.nan, F32), 1)
    assert lab.min() >= 0 and lab.max() < 5


def test_bad_arguments_are_refused_before_any_launch(gpu_ctx, pkg):
    L = pkg.capi.load()
    h = gpu_ctx.h
    with gpu_ctx.scope() as s:
        src = s.put(np.arange(1024, dtype=F32))
        out_f, out_q = s.alloc(4096), s.alloc(4096)
        gpu_ctx.check(L.plhip_memset(h, out_f, 0x55, 4096), "memset")
        gpu_ctx.check(L.plhip_memset(h, out_q, 0x55, 4096), "memset")
        null = C.c_void_p()
        big = (1 << 15) + 1

        def refused(fn, words, *args):
            st = getattr(L, fn)(h, *args)
            msg = L.plhip_last_error(h).decode()
            assert st < 0 and msg.startswith(fn + ": ") and words in msg, (fn, st, msg, words)

        # plhip_interp_f32(x, planes, in_h, in_w, out_h, out_w, method, align_corners, align_mode, y_f32, y_i8, calib_scale)
        fn = "plhip_interp_f32"
        refused(fn, "null", null, 2, 4, 4, 8, 8, 0, 0, 1, out_f, out_q, 1.0)
        refused(fn, "one output is required", src, 2, 4, 4, 8, 8, 0, 0, 1, null, null, 1.0)
        for k in range(5):
            dims = [2, 4, 4, 8, 8]
            dims[k] = 0
            refused(fn, "at least 1", src, *dims, 0, 0, 1, out_f, out_q, 1.0)
            if k:
                dims[k] = big
                refused(fn, "2^15", src, *dims, 0, 0, 1, out_f, out_q, 1.0)
        refused(fn, "unknown method", src, 2, 4, 4, 8, 8, 2, 0, 1, out_f, out_q, 1.0)
        refused(fn, "unknown method", src, 2, 4, 4, 8, 8, -1, 0, 1, out_f, out_q, 1.0)
        refused(fn, "align_mode", src, 2, 4, 4, 8, 8, 0, 0, 2, out_f, out_q, 1.0)
        refused(fn, "align_corners", src, 2, 4, 4, 8, 8, 0, 2, 1, out_f, out_q, 1.0)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(fn, "calib_scale", src, 2, 4, 4, 8, 8, 0, 0, 1, out_f, out_q, bad)
        refused(fn, "2^40", src, 1 << 30, 4, 4, 1 << 10, 1 << 10, 0, 0, 1, out_f, out_q, 1.0)
        refused(fn, "2^40", src, 1 << 30, 1 << 10, 1 << 10, 4, 4, 0, 0, 1, out_f, out_q, 1.0)
        # plhip_arg_max_f32(x, outer, c, inner, y, dtype)
        fn = "plhip_arg_max_f32"
        refused(fn, "null", null, 2, 4, 8, out_f, -1)
        refused(fn, "null", src, 2, 4, 8, null, -1)
        for dims in ((0, 4, 8), (2, 0, 8), (2, 4, 0), (-1, 4, 8)):
            refused(fn, "at least 1", src, *dims, out_f, -1)
        refused(fn, "2^15", src, 2, big, 8, out_f, -1)
        for bad in (0, 1, 4, -2):
            refused(fn, "dtype", src, 2, 4, 8, out_f, bad)
        refused(fn, "2^40", src, 1 << 30, 4, 1 << 30, out_f, -1)
        refused(fn, "2^40", src, 1 << 41, 4, 8, out_f, -1)
        # plhip_interp_argmax_f32(x, n, c, in_h, in_w, out_h, out_w, method, align_corners, align_mode, y, dtype)
        fn = "plhip_interp_argmax_f32"
        refused(fn, "null", null, 2, 4, 4, 4, 8, 8, 0, 0, 1, out_f, -1)
        refused(fn, "null", src, 2, 4, 4, 4, 8, 8, 0, 0, 1, null, -1)
        for k in range(6):
            dims = [2, 4, 4, 4, 8, 8]
            dims[k] = 0
            refused(fn, "at least 1", src, *dims, 0, 0, 1, out_f, -1)
            if k:
                dims[k] = big
                refused(fn, "2^15", src, *dims, 0, 0, 1, out_f, -1)
        refused(fn, "unknown method", src, 2, 4, 4, 4, 8, 8, 7, 0, 1, out_f, -1)
        refused(fn, "align_mode", src, 2, 4, 4, 4, 8, 8, 0, 0, -1, out_f, -1)
        refused(fn, "dtype", src, 2, 4, 4, 4, 8, 8, 0, 0, 1, out_f, 5)
        refused(fn, "2^40", src, 1 << 20, 1 << 10, 4, 4, 1 << 10, 1 << 10, 0, 0, 1, out_f, -1)
        gpu_ctx.sync()
        # nothing was launched: both outputs still hold the fill
        assert (gpu_ctx.to_host(out_f, (4096,), np.uint8) == 0x55).all() and (gpu_ctx.to_host(out_q, (4096,), np.uint8) == 0x55).all()
        # and the same calls with good arguments are taken: 2 planes of 4 x 4 -> 8 x 8 nearest doubles every pixel
        assert L.plhip_interp_f32(h, src, 2, 4, 4, 8, 8, 1, 0, 1, out_f, out_q, 1.0) == 0
        gpu_ctx.sync()
        want = np.arange(32, dtype=F32).reshape(2, 4, 4).repeat(2, axis=1).repeat(2, axis=2)
        assert np.array_equal(gpu_ctx.to_host(out_f, (2, 8, 8), F32), want) and np.array_equal(gpu_ctx.to_host(out_q, (2, 8, 8), np.int8), want.astype(np.int8))
        assert L.plhip_interp_argmax_f32(h, src, 2, 4, 4, 4, 8, 8, 0, 0, 1, out_f, 2) == 0   # the values grow with the channel
        assert L.plhip_arg_max_f32(h, src, 2, 4, 8, out_q, 2) == 0
        gpu_ctx.sync()
        assert (gpu_ctx.to_host(out_f, (2, 8, 8), np.int32) == 3).all() and (gpu_ctx.to_host(out_q, (2, 8), np.int32) == 3).all()


def test_kernel_classes_through_the_factory(lite):
    rng = np.random.default_rng(585)
    scale = SCALES[0]
    x = _inputs(rng, (2, 6, 5, 7), scale, nonfinite=True)
    logits = _with_ties(rng, rng.standard_normal((2, 19, 8, 8)).astype(F32), 1)
    p = lite.Predictor(0)
    try:
        for name, v in (("x", x), ("logits", logits)):
            p.add_feed(name, v.shape)
            p.add_io_copy(name, name + "d", True)
        p.add_interp("bilinear_interp", "xd", "bil", (10, 21), 0.0, False, 1)
        p.add_interp("bilinear_interp", "xd", "bil0", (10, 21), 0.0, False, 0)
        p.add_interp("nearest_interp", "xd", "near", None, 2.0, True, 1)                     # by scale: 10 x 14
        p.add_interp("bilinear_interp", "xd", "bil_f", (10, 21), 0.0, False, 1, "bil_q", scale, False)
        p.add_interp("nearest_interp", "xd", "near_dropped", None, 2.0, True, 1, "near_q", scale, True)
        p.add_calib("bil", "bil_sep_q", scale, True)
        p.add_calib("near", "near_sep_q", scale, True)
        p.add_interp("bilinear_interp", "logitsd", "up", (32, 32), 0.0, True, 1)
        p.add_arg_max("up", "lab64", 1, -1, False)
        p.add_arg_max("up", "lab32k", 1, 2, True)
        p.add_arg_max("up", "lab_w", -1, 3, False)
        p.add_interp_arg_max("bilinear_interp", "logitsd", "fused64", (32, 32), 0.0, True, 1, -1, False)
        p.add_interp_arg_max("bilinear_interp", "logitsd", "fused32k", None, 4.0, True, 1, 2, True)
        for name in ("lab64", "lab32k", "fused64", "fused32k"):
            p.add_io_copy(name, name + "/host", False)
        p.set_input("x", x)
        p.set_input("logits", logits)
        p.run()
        p.run()
        names = "\n".join(p.kernel_names())
        assert names.count("/def -> bilinear_interp_hip") == 3 and names.count("/def -> nearest_interp_hip") == 1, names
        assert "/int8 -> bilinear_interp_fp32_int8_hip" in names and "/int8 -> nearest_interp_int8_hip" in names, names
        assert names.count("/def -> arg_max_hip") == 3 and names.count("/interp -> bilinear_interp_arg_max_hip") == 2, names
        # NaN and infinities are planted in x: compared as bits where the oracle has numbers, and against the separate instructions everywhere
        num = lambda a: ~np.isnan(a)
        for var, want in (("bil", I.interp(x, (10, 21), "bilinear", False, 1)), ("bil0", I.interp(x, (10, 21), "bilinear", False, 0)),
                          ("near", I.interp(x, (10, 14), "nearest", True, 1))):
            got = p.get_var(var, F32)
            assert got.shape == want.shape and np.array_equal(_bits(got)[num(want)], _bits(want)[num(want)]), var
        assert p.get_var("bil_f", F32).tobytes() == p.get_var("bil", F32).tobytes()
        assert p.get_var("bil_q", np.int8).tobytes() == p.get_var("bil_sep_q", np.int8).tobytes()
        assert p.get_var("near_q", np.int8).tobytes() == p.get_var("near_sep_q", np.int8).tobytes()
        want = I.interp(x, (10, 21), "bilinear", False, 1)
        assert np.array_equal(p.get_var("bil_q", np.int8)[num(want)], S.calib_i8(want, scale)[num(want)])
        up = I.interp(logits, (32, 32), "bilinear", True, 1)
        assert _tied(up, 1) > 0 and np.array_equal(_bits(p.get_var("up", F32)), _bits(up))
        for var, dtype, keep, np_t in (("lab64", -1, False, np.int64), ("lab32k", 2, True, np.int32), ("fused64", -1, False, np.int64),
                                       ("fused32k", 2, True, np.int32)):
            want = I.arg_max(up, 1, dtype, keep)
            for name in (var, var + "/host"):       # an int64 / int32 variable is fetched like any other: io_copy, get_var
                got = p.get_var(name, np_t)
                assert got.shape == want.shape and np.array_equal(got, want), name
        assert np.array_equal(p.get_var("lab_w", np.int64), I.arg_max(up, -1, 3))
    finally:
        p.close()


def test_kernel_classes_are_fatal_on_what_they_do_not_take(lite):
    for kw, words in ((dict(out_hw=None, scale=0.0), "neither out_h / out_w nor a scale"), (dict(out_hw=(4, 4), align_mode=2), "align_mode")):
        p = lite.Predictor(0)
        try:
            p.add_feed("x", (1, 2, 3, 3))
            p.add_io_copy("x", "xd", True)
            p.add_interp("bilinear_interp", "xd", "y", **kw)
            p.set_input("x", np.zeros((1, 2, 3, 3), F32))
            with pytest.raises(lite.LiteError) as e:
                p.run()
            assert words in str(e.value), str(e.value)
        finally:
            p.close()
    for dtype in (0, 1, 5):
        p = lite.Predictor(0)
        try:
            p.add_feed("x", (1, 2, 3, 3))
            p.add_io_copy("x", "xd", True)
            p.add_arg_max("xd", "y", 1, dtype, False)
            p.set_input("x", np.zeros((1, 2, 3, 3), F32))
            with pytest.raises(lite.LiteError) as e:
                p.run()
            assert "dtype" in str(e.value), str(e.value)
        finally:
            p.close()
