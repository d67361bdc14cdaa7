"""GPU: plhip_conv2d_transpose_int8 (deconv_i8.hip) through the C ABI against tests/deconv_oracle.py, operands from
edge_cases.py (dyadic folded scales, quarter biases, outputs pinned on rounding ties and the saturation bounds).

int32 accumulators and int8 outputs bit for bit, fp32 within rtol 1e-5.  Every case asserts the route's name first, and every
case of the MFMA phase route runs a second time through the direct route (knob DECONV_ROUTE = 1) and must give the same bytes in
all three output kinds.  Shapes are the smallest at which a path of the phase kernel changes: a lane unit is 4 output columns
and 1 (stride 1) or 2 (stride 2) output rows, a wave holds 32 units, a block 128, a segment 32 units of a row, a K chunk 32
input channels, an M tile 32 output channels."""
import ctypes

import numpy as np
import pytest

import deconv_oracle as D
import edge_cases as E
from test_deconv_host import DIRECT, PHASE, pack_ref

pytestmark = pytest.mark.gpu


class _DirectRoute:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        assert self.lib.plhip_debug_set(b"DECONV_ROUTE", 1) == 0

    def __exit__(self, *a):
        self.lib.plhip_debug_set(b"DECONV_ROUTE", 0)


def _route(cin, kh, kw, pads, st, dl, g):
    inside = (g == 1 and cin % 32 == 0 and dl == (1, 1) and kh <= 4 and kw <= 4 and st in ((1, 1), (2, 2)) and
              max(pads[0], pads[1]) < kh and max(pads[2], pads[3]) < kw)
    return PHASE if inside else DIRECT


def _case(plref, seed, n, cin, h, w, cout, kh, kw, pads, st, dl=(1, 1), g=1, act=E.ACT_NONE, alpha=0.0, osz=(0, 0), x=None, wt=None,
          bias=True):
    """Operands and the oracle's three outputs of one transposed conv."""
    rng = np.random.default_rng(seed)
    es, ts = E.channel_plan(cout)
    k = max(1, cin // g * max(1, kh // st[0]) * max(1, kw // st[1]))  # products per output, about
    if x is None:
        x = E.activations(rng, (n, cin, h, w))
    if wt is None:  # drawn per OUTPUT channel, stored [cin][cout / g][kh][kw]
        wo = E.weights(rng, (cout, cin // g, kh, kw), k, es, ts)
        wt = np.ascontiguousarray(wo.reshape(g, cout // g, cin // g, kh, kw).transpose(0, 2, 1, 3, 4).reshape(cin, cout // g, kh, kw))
    acc = D.acc_gather(x, wt, pads, st, dl, g, osz)
    sc, bi = E.fold(rng, acc, es, act, alpha)
    b0 = bi if bias else np.zeros(cout, np.float32)
    return dict(x=x, w=wt, acc=acc, scale=sc, bias=bi if bias else None, i8=plref.epilogue(acc, sc, b0, act, alpha, True),
                f32=plref.epilogue(acc, sc, b0, act, alpha, False),
                desc=(n, cin, h, w, cout, kh, kw, pads, st, dl, g, act, alpha, osz))


def _run3(ctx, capi, d, c):
    return [ctx.conv2d_transpose(d, c["x"], c["w"], s, b, ok)
            for ok, s, b in ((capi.OUT_I32, None, None), (capi.OUT_I8, c["scale"], c["bias"]), (capi.OUT_F32, c["scale"], c["bias"]))]


def _check(ctx, capi, c, what=""):
    n, cin, h, w, cout, kh, kw, pads, st, dl, g, act, alpha, osz = c["desc"]
    d = capi.deconv_desc(n, cin, h, w, cout, kh, kw, pads, st, dl, g, act, alpha, osz)
    want = _route(cin, kh, kw, pads, st, dl, g)
    what = "%s %s" % (what, c["desc"])
    assert capi.deconv_impl_name(d) == want, what
    assert capi.deconv_out_hw(d) == c["acc"].shape[2:], what
    got = _run3(ctx, capi, d, c)
    assert np.array_equal(got[0], c["acc"]), "%s int32: %d differ" % (what, (got[0] != c["acc"]).sum())
    assert np.array_equal(got[1], c["i8"]), "%s int8: %d differ" % (what, (got[1] != c["i8"]).sum())
    np.testing.assert_allclose(got[2], c["f32"], rtol=1e-5, atol=0, err_msg=what + " fp32")
    if want == PHASE:  # A/B: the direct route on the same operands gives the same bytes
        with _DirectRoute(ctx.L):
            assert capi.deconv_impl_name(d) == DIRECT
            other = _run3(ctx, capi, d, c)
        assert capi.deconv_impl_name(d) == PHASE
        for a, b in zip(got, other):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what + " phase != direct"


# ---- the phase route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_kernel_by_stride_by_pads(gpu_ctx, pkg, plref, k, s):
    capi = pkg.capi
    for i, pads in enumerate(((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 1, 0), (k - 1,) * 4)):
        _check(gpu_ctx, capi, _case(plref, 100 * k + 10 * s + i, 2, 32, 5, 9, 32, k, k, pads, (s, s), act=E.ACT_RELU))


@pytest.mark.parametrize("s", [1, 2])
def test_one_hot_input_reproduces_the_filter(gpu_ctx, pkg, s):
    """x is 1 at one (image, channel, pixel): the accumulators are the filter of that input channel, unflipped, at
    (iy s - pt + r, ix s - pl + s_) -- stated here without the oracle."""
    capi = pkg.capi
    n, cin, h, w, cout, k, pads = 2, 64, 4, 6, 5, 4, (1, 2, 2, 1)
    wt = ((np.arange(cin * cout * k * k) * 37) % 251 - 125).astype(np.int8).reshape(cin, cout, k, k)
    assert len(set(wt[40].ravel().tolist())) == cout * k * k  # all distinct
    d = capi.deconv_desc(n, cin, h, w, cout, k, k, pads, (s, s))
    assert capi.deconv_impl_name(d) == PHASE
    oh, ow = capi.deconv_out_hw(d)
    for iy, ix in ((0, 0), (2, 3), (3, 5)):
        x = np.zeros((n, cin, h, w), np.int8)
        x[1, 40, iy, ix] = 1
        want = np.zeros((n, cout, oh, ow), np.int32)
        for r in range(k):
            for q in range(k):
                oy, ox = iy * s - pads[0] + r, ix * s - pads[2] + q
                if 0 <= oy < oh and 0 <= ox < ow:
                    want[1, :, oy, ox] = wt[40, :, r, q]
        assert want.any()
        got = gpu_ctx.conv2d_transpose(d, x, wt, None, None, capi.OUT_I32)
        assert np.array_equal(got, want), (s, iy, ix)


@pytest.mark.parametrize("cin", [32, 64, 96])
def test_k_chunks_and_the_m_tail(gpu_ctx, pkg, plref, cin):
    capi = pkg.capi
    for cout in (1, 21, 32, 33, 64):
        _check(gpu_ctx, capi, _case(plref, 2000 + cin + cout, 2, cin, 4, 5, cout, 3, 3, (1, 1, 1, 1), (2, 2), act=E.ACT_LEAKY, alpha=0.25))


@pytest.mark.parametrize("h,w", [(2, 1), (2, 3), (2, 17), (2, 33), (2, 65), (1, 33), (37, 3), (37, 65)])
def test_column_and_row_tails(gpu_ctx, pkg, plref, h, w):
    """k 4 s 2 p 1: OW = 2 W crosses a quad (W 3), a wave's 32 units (17), a row of 32 units = one segment (33 -> 66 columns
    stay in it, 65 -> 130 columns = 33 units cross into a second segment); H 37 crosses band boundaries.  The same planes at
    stride 1 (k 3 p 1), where a unit is 4 input columns."""
    capi = pkg.capi
    _check(gpu_ctx, capi, _case(plref, 3000 + 70 * h + w, 1, 32, h, w, 32, 4, 4, (1, 1, 1, 1), (2, 2)))
    _check(gpu_ctx, capi, _case(plref, 3500 + 70 * h + w, 1, 32, h, w, 32, 3, 3, (1, 1, 1, 1), (1, 1)))


def test_wide_rows_cross_segments_at_stride_1(gpu_ctx, pkg, plref):
    capi = pkg.capi
    _check(gpu_ctx, capi, _case(plref, 3900, 1, 32, 3, 131, 32, 3, 3, (1, 1, 1, 1), (1, 1)))


@pytest.mark.parametrize("eh,ew", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_output_size(gpu_ctx, pkg, plref, eh, ew):
    capi = pkg.capi
    for k, pads in ((2, (0, 0, 0, 0)), (3, (1, 1, 1, 1)), (4, (1, 1, 1, 1))):
        oh, ow = D.out_dims(5, 9, k, k, pads, (2, 2), (1, 1))
        osz = (oh + eh if eh else 0, ow + ew if ew else 0)
        c = _case(plref, 4000 + 10 * k + 2 * eh + ew, 2, 32, 5, 9, 32, k, k, pads, (2, 2), osz=osz)
        assert c["acc"].shape[2:] == (oh + eh, ow + ew)
        _check(gpu_ctx, capi, c)


@pytest.mark.parametrize("n", [1, 3])
def test_batch(gpu_ctx, pkg, plref, n):
    capi = pkg.capi
    _check(gpu_ctx, capi, _case(plref, 4500 + n, n, 64, 6, 7, 40, 2, 2, (0, 0, 0, 0), (2, 2)))
    _check(gpu_ctx, capi, _case(plref, 4510 + n, n, 64, 6, 7, 40, 3, 3, (1, 1, 1, 1), (1, 1)))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("act,alpha", [(E.ACT_NONE, 0.0), (E.ACT_RELU, 0.0), (E.ACT_RELU6, 60.0), (E.ACT_RELU6, 60.5),
                                       (E.ACT_LEAKY, 0.25)])
def test_activations(gpu_ctx, pkg, plref, act, alpha, bias):
    capi = pkg.capi
    for s, k, pads in ((2, 4, (1, 1, 1, 1)), (1, 3, (1, 1, 1, 1)), (2, 2, (0, 0, 0, 0))):
        c = _case(plref, 5000 + act * 7 + s + k, 2, 64, 5, 9, 40, k, k, pads, (s, s), act=act, alpha=alpha, bias=bias)
        if act == E.ACT_RELU6:  # the clip is visible in the int8 output
            q = int(alpha + 0.5)
            assert (c["f32"] == np.float32(alpha)).any() and (c["i8"] == q).any() and c["i8"].max() == q < 127
        _check(gpu_ctx, capi, c, "act %d" % act)


def test_maximum_magnitude(gpu_ctx, pkg, plref):
    """x = -128 and w = -127 over Cin 96 and all 9 taps: the accumulators are exact, and with a scale that brings them to about
    200 LSB and a bias of -400 on every other channel the int8 output saturates at both ends."""
    capi = pkg.capi
    n, cin, h, w, cout = 2, 96, 5, 9, 33
    x = np.full((n, cin, h, w), -128, np.int8)
    wt = np.full((cin, cout, 3, 3), -127, np.int8)
    acc = D.acc_gather(x, wt, (1, 1, 1, 1), (1, 1), (1, 1))
    assert acc.max() == 96 * 9 * 128 * 127
    sc = np.full(cout, 2.0 ** -16, np.float32)
    bi = np.where(np.arange(cout) % 2 == 1, -400.0, 0.25).astype(np.float32)
    c = dict(x=x, w=wt, acc=acc, scale=sc, bias=bi, i8=plref.epilogue(acc, sc, bi, 0, 0.0, True),
             f32=plref.epilogue(acc, sc, bi, 0, 0.0, False), desc=(n, cin, h, w, cout, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 1, 0, 0.0, (0, 0)))
    assert c["i8"].max() == 127 and c["i8"].min() == -127 and c["f32"].max() > 127.5 and c["f32"].min() < -127.5
    _check(gpu_ctx, capi, c, "max magnitude")
    xm, wm = E.maxmag_operands(np.random.default_rng(78), (n, cin, h, w), (cout, cin, 3, 3))
    _check(gpu_ctx, capi, _case(plref, 79, n, cin, h, w, cout, 3, 3, (1, 1, 1, 1), (1, 1), x=xm,
                                wt=np.ascontiguousarray(wm.transpose(1, 0, 2, 3))), "maxmag operands")


@pytest.mark.parametrize("s", [1, 2])
def test_unaligned_output(gpu_ctx, pkg, plref, s):
    """y 1, 2 and 3 bytes (int8) / elements (fp32, int32) into its buffer: the same values, the sentinel bytes in front of and
    behind the tensor untouched.  k 4 p 1 at stride 2 and k 3 p 1 at stride 1 start every row's quads one column left of the
    tensor, so the store paths with `skip` and with a short last quad are on both sides of every row."""
    capi = pkg.capi
    k = 4 if s == 2 else 3
    for h, w in ((4, 8), (5, 9)):
        c = _case(plref, 6000 + s + h, 2, 32, h, w, 33, k, k, (1, 1, 1, 1), (s, s), act=E.ACT_RELU)
        n, cin, _, _, cout = c["desc"][:5]
        d = capi.deconv_desc(n, cin, h, w, cout, k, k, (1, 1, 1, 1), (s, s), act=E.ACT_RELU)
        assert capi.deconv_impl_name(d) == PHASE
        for off in (1, 2, 3):
            y, around = gpu_ctx.conv2d_transpose(d, c["x"], c["w"], c["scale"], c["bias"], capi.OUT_I8, misalign=off, sentinel=0xA5)
            assert np.array_equal(y, c["i8"]) and (around == 0xA5).all(), (s, h, w, off)
            y, around = gpu_ctx.conv2d_transpose(d, c["x"], c["w"], c["scale"], c["bias"], capi.OUT_F32, misalign=4 * off, sentinel=0xA5)
            np.testing.assert_allclose(y, c["f32"], rtol=1e-5, atol=0)
            assert (around == 0xA5).all(), (s, h, w, off)
            y, around = gpu_ctx.conv2d_transpose(d, c["x"], c["w"], None, None, capi.OUT_I32, misalign=4 * off, sentinel=0xA5)
            assert np.array_equal(y, c["acc"]) and (around == 0xA5).all(), (s, h, w, off)


@pytest.mark.parametrize("cin,cout,kh,kw", [(32, 32, 2, 2), (64, 21, 3, 3), (96, 33, 4, 4), (32, 1, 1, 1), (64, 64, 4, 2)])
def test_device_packer_equals_the_host_restatement(gpu_ctx, pkg, cin, cout, kh, kw):
    capi, C = pkg.capi, ctypes
    d = capi.deconv_desc(1, cin, 4, 4, cout, kh, kw, (0, 0, 0, 0), (2, 2))
    assert capi.deconv_impl_name(d) == PHASE
    w = np.random.default_rng(cin + cout).integers(-128, 128, (cin, cout, kh, kw)).astype(np.int8)
    nbytes = gpu_ctx.L.plhip_deconv_packed_weight_bytes(C.byref(d))
    shape = (-(-cout // 32), cin // 32, kh * kw, 64, 16)
    assert nbytes == int(np.prod(shape))
    dw, dwp = gpu_ctx.to_device(w), gpu_ctx.malloc(nbytes)
    gpu_ctx.check(gpu_ctx.L.plhip_pack_deconv_weights(gpu_ctx.h, C.byref(d), dw, dwp), "pack")
    got = gpu_ctx.to_host(dwp, shape, np.int8)
    gpu_ctx.free(dw), gpu_ctx.free(dwp)
    assert np.array_equal(got, pack_ref(w, cin, cout, kh, kw))


# ---- the direct route -------------------------------------------------------------------------------------------------------------
DIRECT_CASES = {
    "groups 2": (2, 8, 5, 6, 12, 3, 3, (1, 1, 1, 1), (2, 2), (1, 1), 2),
    "depthwise k4 s2 p1": (2, 8, 5, 6, 8, 4, 4, (1, 1, 1, 1), (2, 2), (1, 1), 8),
    "dilation 2": (2, 32, 5, 6, 16, 3, 3, (2, 2, 2, 2), (1, 1), (2, 2), 1),
    "stride 3": (2, 32, 4, 5, 16, 3, 3, (0, 1, 1, 0), (3, 3), (1, 1), 1),
    "stride (2,1)": (2, 32, 4, 5, 16, 3, 3, (1, 1, 1, 1), (2, 1), (1, 1), 1),
    "k 5": (2, 32, 4, 5, 16, 5, 5, (2, 2, 2, 2), (2, 2), (1, 1), 1),
    "cin 3": (2, 3, 6, 7, 16, 4, 4, (1, 1, 1, 1), (2, 2), (1, 1), 1),
    "k16 s8 p4 (FCN-8s head)": (1, 5, 3, 3, 5, 16, 16, (4, 4, 4, 4), (8, 8), (1, 1), 1),
}


@pytest.mark.parametrize("what", sorted(DIRECT_CASES))
def test_direct_route(gpu_ctx, pkg, plref, what):
    capi = pkg.capi
    n, cin, h, w, cout, kh, kw, pads, st, dl, g = DIRECT_CASES[what]
    for i, (act, alpha) in enumerate(((E.ACT_NONE, 0.0), (E.ACT_RELU6, 60.5), (E.ACT_LEAKY, 0.25))):
        c = _case(plref, 7000 + 10 * sorted(DIRECT_CASES).index(what) + i, n, cin, h, w, cout, kh, kw, pads, st, dl, g, act, alpha,
                  bias=i != 2)
        assert _route(cin, kh, kw, pads, st, dl, g) == DIRECT
        _check(gpu_ctx, capi, c, what)


def test_direct_route_output_size(gpu_ctx, pkg, plref):
    capi = pkg.capi
    oh, ow = D.out_dims(4, 5, 3, 3, (0, 1, 1, 0), (3, 3), (1, 1))
    _check(gpu_ctx, capi, _case(plref, 7900, 2, 6, 4, 5, 4, 3, 3, (0, 1, 1, 0), (3, 3), g=2, osz=(oh + 2, ow + 1)))


def test_refusals_on_the_device(gpu_ctx, pkg):
    capi, C = pkg.capi, ctypes
    d = capi.deconv_desc(1, 32, 4, 4, 32, 2, 2, (0, 0, 0, 0), (2, 2))
    one = gpu_ctx.malloc(64)
    L, h = gpu_ctx.L, gpu_ctx.h
    assert L.plhip_conv2d_transpose_int8(h, C.byref(d), one, one, one, None, one, capi.OUT_F32_GAP) == -1
    assert "bad out kind" in L.plhip_last_error(h).decode()
    assert L.plhip_conv2d_transpose_int8(h, C.byref(d), one, one, None, None, one, capi.OUT_I8) == -1
    assert "scale required" in L.plhip_last_error(h).decode()
    bad = capi.deconv_desc(1, 32, 4, 4, 32, 2, 2, (0, 0, 0, 0), (2, 2), output_size=(10, 0))
    assert L.plhip_conv2d_transpose_int8(h, C.byref(bad), one, one, one, None, one, capi.OUT_I8) == -1
    assert "output size outside" in L.plhip_last_error(h).decode()
    assert L.plhip_pack_deconv_weights(h, C.byref(bad), one, one) == -1
    gpu_ctx.free(one)
