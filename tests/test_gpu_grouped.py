"""GPU: the grouped 3x3 route (conv_grouped_i8.hip) through the C ABI against the oracle, operands from edge_cases.py.

int32 accumulators and int8 outputs bit for bit, fp32 within rtol 1e-5.  Every case asserts the route's name first, so nothing
falls back to im2col silently.

Channel counts: the route's envelope is groups >= 4 with Cg in {4, 8, 16, 32}, so cin = 32 exists for Cg 4 / 8 only, 64 from
Cg 16 down, and Cg = 32 starts at cin = 128.  CINS gives every Cg its smallest channel count, a second one, and a chunk count
(cin / 32) that is no power of two: 1 / 2 / 3 chunks where the envelope has them, else the nearest ones inside it."""
import ctypes

import numpy as np
import pytest

import edge_cases as E
from test_grouped_route_host import GROUPED, IM2COL, pack_ref

pytestmark = pytest.mark.gpu

CINS = {4: (32, 64, 96), 8: (32, 64, 96), 16: (64, 96, 160), 32: (128, 160, 192)}
SMALL_PLANES = ((7, 7), (14, 14), (9, 13), (3, 3), (2, 2))  # smaller than any tile; odd, width no multiple of 4; a single output at stride 2
LARGE_PLANES = ((28, 28), (56, 56))                          # band tails, the workload's planes: at the smallest cin only
P1 = (1, 1, 1, 1)


def _shape(n, cin, h, w, cg, pads, st):
    return (n, cin, h, w, cin, 3, 3, pads, st, 1, cin // cg)


def _desc(capi, shape, act=E.ACT_NONE, alpha=0.0):
    n, cin, h, w, cout, kh, kw, pads, st, dl, g = shape
    return capi.conv_desc(n, cin, h, w, cout, kh, kw, pads, (st, st), (dl, dl), g, act, alpha)


def _named(ctx, d, want=GROUPED):
    assert ctx.L.plhip_conv_impl_name(ctypes.byref(d)).decode() == want


def _case(plref, shape, act, alpha, seed, x=None, w=None, bias=True):
    """Operands (edge_cases generators) and the oracle's three outputs of one conv."""
    n, cin, h, wd, cout, kh, kw, pads, st, dl, g = shape
    rng = np.random.default_rng(seed)
    es, ts = E.channel_plan(cout)
    k = cin // g * 9
    if x is None:
        x = E.activations(rng, (n, cin, h, wd))
    if w is None:
        w = E.weights(rng, (cout, cin // g, 3, 3), k, es, ts)
    acc = plref.conv2d_acc(plref.shape(n, cin, h, wd, cout, kh, kw, pads, (st, st), (dl, dl), g), x, w)
    sc, bi = E.fold(rng, acc, es, act, alpha)
    if not bias:
        bi = None
    b0 = bi if bias else np.zeros(cout, np.float32)
    return dict(x=x, w=w, acc=acc, scale=sc, bias=bi, i8=plref.epilogue(acc, sc, b0, act, alpha, True),
                f32=plref.epilogue(acc, sc, b0, act, alpha, False))


def _check(ctx, capi, d, c, what):
    _named(ctx, d)
    got = ctx.conv2d(d, c["x"], c["w"], None, None, capi.OUT_I32)
    assert np.array_equal(got, c["acc"]), "%s int32: %d differ" % (what, (got != c["acc"]).sum())
    got = ctx.conv2d(d, c["x"], c["w"], c["scale"], c["bias"], capi.OUT_I8)
    assert np.array_equal(got, c["i8"]), "%s int8: %d differ" % (what, (got != c["i8"]).sum())
    got = ctx.conv2d(d, c["x"], c["w"], c["scale"], c["bias"], capi.OUT_F32)
    np.testing.assert_allclose(got, c["f32"], rtol=1e-5, atol=0, err_msg=what + " fp32")


@pytest.mark.parametrize("st", [1, 2])
@pytest.mark.parametrize("cg", [4, 8, 16, 32])
def test_cg_by_stride(gpu_ctx, pkg, plref, cg, st):
    capi, seed = pkg.capi, 100 * cg + st
    for ci, cin in enumerate(CINS[cg]):
        for h, w in SMALL_PLANES + (LARGE_PLANES if ci == 0 else ()):
            for n in (1, 2, 3):
                shape = _shape(n, cin, h, w, cg, P1, st)
                seed += 1
                _check(gpu_ctx, capi, _desc(capi, shape, E.ACT_RELU), _case(plref, shape, E.ACT_RELU, 0.0, seed), str(shape))


@pytest.mark.parametrize("st", [1, 2])
@pytest.mark.parametrize("pads", [(1, 1, 1, 1), (0, 0, 0, 0), (0, 1, 0, 1), (1, 0, 1, 0)])
def test_pads(gpu_ctx, pkg, plref, pads, st):
    capi = pkg.capi
    for i, (cg, cin, h, w) in enumerate(((4, 32, 9, 13), (8, 64, 14, 14), (16, 96, 7, 7), (32, 128, 10, 8), (8, 32, 30, 57))):
        shape = _shape(2, cin, h, w, cg, pads, st)
        _check(gpu_ctx, capi, _desc(capi, shape), _case(plref, shape, E.ACT_NONE, 0.0, 900 + 10 * sum(pads) + i + st), str(shape))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("act,alpha", [(E.ACT_NONE, 0.0), (E.ACT_RELU, 0.0), (E.ACT_RELU6, 60.0), (E.ACT_RELU6, 60.5),
                                       (E.ACT_LEAKY, 0.25)])
def test_activations(gpu_ctx, pkg, plref, act, alpha, bias):
    capi = pkg.capi
    for st, (cg, cin) in ((1, (8, 64)), (2, (4, 96)), (1, (32, 128))):
        shape = _shape(2, cin, 9, 13, cg, P1, st)
        c = _case(plref, shape, act, alpha, 300 + act * 7 + st + cg, bias=bias)
        if act == E.ACT_RELU6:  # the clip is visible in the int8 output
            q = int(alpha + 0.5)
            assert (c["f32"] == np.float32(alpha)).any() and (c["i8"] == q).any() and c["i8"].max() == q < 127
        _check(gpu_ctx, capi, _desc(capi, shape, act, alpha), c, "%s act %d" % (shape, act))


@pytest.mark.parametrize("st", [1, 2])
@pytest.mark.parametrize("cg", [4, 8, 16, 32])
def test_no_leak_between_groups(gpu_ctx, pkg, plref, cg, st):
    """Input non-zero in the channels of ONE group, every weight +-127: each output channel outside that group equals its
    bias-only value exactly (a wrong diagonal block cannot hide behind random data)."""
    capi = pkg.capi
    cin = CINS[cg][1]
    rng = np.random.default_rng(4000 + cg + st)
    for grp in (0, cin // cg - 1, (cin // cg) // 2 + 1):
        shape = _shape(2, cin, 9, 13, cg, P1, st)
        x = np.zeros((2, cin, 9, 13), np.int8)
        x[:, grp * cg:(grp + 1) * cg] = E.activations(rng, (2, cg, 9, 13))
        w = rng.choice(np.array([-127, 127], np.int8), (cin, cg, 3, 3))
        c = _case(plref, shape, E.ACT_NONE, 0.0, 4100 + grp, x=x, w=w)
        d = _desc(capi, shape)
        _check(gpu_ctx, capi, d, c, "leak %s group %d" % (shape, grp))
        outside = np.ones(cin, bool)
        outside[grp * cg:(grp + 1) * cg] = False
        acc = gpu_ctx.conv2d(d, x, w, None, None, capi.OUT_I32)
        assert not acc[:, outside].any() and acc[:, ~outside].any()
        zero = np.zeros_like(c["acc"])
        y8 = gpu_ctx.conv2d(d, x, w, c["scale"], c["bias"], capi.OUT_I8)
        assert np.array_equal(y8[:, outside], plref.epilogue(zero, c["scale"], c["bias"], 0, 0.0, True)[:, outside])
        yf = gpu_ctx.conv2d(d, x, w, c["scale"], c["bias"], capi.OUT_F32)
        assert np.array_equal(yf[:, outside], np.broadcast_to(c["bias"][None, :, None, None], yf.shape)[:, outside])


@pytest.mark.parametrize("st", [1, 2])
def test_maximum_magnitude(gpu_ctx, pkg, plref, st):
    """x = 127 and w = +-127 over the full K = 288 (Cg = 32): the accumulators are exact."""
    capi = pkg.capi
    shape = _shape(2, 128, 9, 13, 32, P1, st)
    rng = np.random.default_rng(77 + st)
    x = np.full((2, 128, 9, 13), 127, np.int8)
    w = np.where(np.arange(128) % 3 == 1, -127, 127).astype(np.int8)[:, None, None, None] * np.ones((1, 32, 3, 3), np.int8)
    acc = plref.conv2d_acc(plref.shape(2, 128, 9, 13, 128, 3, 3, P1, (st, st), (1, 1), 4), x, w)
    assert np.abs(acc).max() == 288 * 127 * 127
    sc, bi = E.fold_maxmag(rng, acc)
    c = dict(x=x, w=w, acc=acc, scale=sc, bias=bi, i8=plref.epilogue(acc, sc, bi, 0, 0.0, True),
             f32=plref.epilogue(acc, sc, bi, 0, 0.0, False))
    _check(gpu_ctx, capi, _desc(capi, shape), c, "max magnitude %s" % (shape,))
    xm, wm = E.maxmag_operands(rng, (2, 128, 9, 13), (128, 32, 3, 3), 4)  # -128 sprinkled through both
    _check(gpu_ctx, capi, _desc(capi, shape), _case(plref, shape, E.ACT_NONE, 0.0, 78, x=xm, w=wm), "maxmag operands")


@pytest.mark.parametrize("st", [1, 2])
def test_fused_tail(gpu_ctx, pkg, plref, st):
    """plhip_conv2d_int8_fused: residual + relu + calib copy, and the calib copy alone (y_f32 = NULL), against the three
    separate oracle steps bit for bit."""
    capi = pkg.capi
    shape = _shape(2, 64, 9, 13, 8, P1, st)
    for act in (E.ACT_NONE, E.ACT_RELU):
        c = _case(plref, shape, act, 0.0, 500 + st + act)
        d = _desc(capi, shape, act)
        _named(gpu_ctx, d)
        rng = np.random.default_rng(510 + st)
        res = (np.round(rng.uniform(-70, 70, c["f32"].shape) * 4) / 4).astype(np.float32)
        z = plref.elementwise_add(c["f32"], res, True)
        yf, yq = gpu_ctx.conv2d_fused(d, c["x"], c["w"], c["scale"], c["bias"], res, 1, 0.5)
        assert np.array_equal(yf.view(np.uint32), z.view(np.uint32))
        assert np.array_equal(yq, plref.calib_f32_to_i8(z, 0.5))
        z = plref.elementwise_add(c["f32"], res, False)  # the residual without the relu
        yf, yq = gpu_ctx.conv2d_fused(d, c["x"], c["w"], c["scale"], c["bias"], res, 0, 0.5)
        assert np.array_equal(yf.view(np.uint32), z.view(np.uint32))
        assert np.array_equal(yq, plref.calib_f32_to_i8(z, 0.5))
        yf, yq = gpu_ctx.conv2d_fused(d, c["x"], c["w"], c["scale"], c["bias"], None, 0, 0.5, want_f32=False)
        assert yf is None and np.array_equal(yq, plref.calib_f32_to_i8(c["f32"], 0.5))


def _conv_at_offset(ctx, capi, d, c, out_kind, off):
    """plhip_conv2d_int8 with y `off` elements into its buffer; returns (the output, the bytes in front of and behind it)."""
    C, L = ctypes, ctx.L
    oh, ow = capi.out_hw(d)
    dt = np.dtype(np.int8 if out_kind == capi.OUT_I8 else np.float32)
    with ctx.scope() as s:
        dx, dw = s.put(c["x"]), s.put(c["w"])
        ds, db = s.put(c["scale"]), s.put(c["bias"])
        y = s.out((d.n, d.cout, oh, ow), dt, off=off * dt.itemsize, fill=0xA5)
        dwp = s.alloc(L.plhip_conv_packed_weight_bytes(C.byref(d)))
        ctx.check(L.plhip_pack_conv_weights(ctx.h, C.byref(d), dw, dwp), "pack")
        assert L.plhip_conv_workspace_bytes(C.byref(d)) == 0
        ctx.check(L.plhip_conv2d_int8(ctx.h, C.byref(d), dx, dwp, ds, db, y.ptr, out_kind, C.c_void_p(), 0), "conv2d")
        return y.get(), y.margins()


@pytest.mark.parametrize("st", [1, 2])
def test_unaligned_output(gpu_ctx, pkg, plref, st):
    """y offset by 1 element (int8) and 1 float (fp32): the same values, nothing written outside the tensor."""
    capi = pkg.capi
    for h, w in ((8, 16), (9, 13)):
        shape = _shape(2, 64, h, w, 16, P1, st)
        c = _case(plref, shape, E.ACT_RELU, 0.0, 600 + st + h)
        d = _desc(capi, shape, E.ACT_RELU)
        _named(gpu_ctx, d)
        for off in (1, 3):
            y, around = _conv_at_offset(gpu_ctx, capi, d, c, capi.OUT_I8, off)
            assert np.array_equal(y, c["i8"]) and (around == 0xA5).all()
            y, around = _conv_at_offset(gpu_ctx, capi, d, c, capi.OUT_F32, off)
            np.testing.assert_allclose(y, c["f32"], rtol=1e-5, atol=0)
            assert (around == 0xA5).all()


class _GroupedOff:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        assert self.lib.plhip_debug_set(b"CONV_GROUPED", 0) == 0

    def __exit__(self, *a):
        self.lib.plhip_debug_set(b"CONV_GROUPED", 1)


@pytest.mark.parametrize("cg", [4, 8, 16, 32])
def test_both_routes_give_the_same_bytes(gpu_ctx, pkg, plref, cg):
    """CONV_GROUPED = 0 runs the im2col route on the same inputs: the same bytes in all three output kinds."""
    capi = pkg.capi
    for st in (1, 2):
        shape = _shape(3, CINS[cg][2], 14, 14, cg, P1, st)
        c = _case(plref, shape, E.ACT_LEAKY, 0.25, 700 + cg + st)
        d = _desc(capi, shape, E.ACT_LEAKY, 0.25)
        _named(gpu_ctx, d)
        outs = ((capi.OUT_I32, None, None), (capi.OUT_I8, c["scale"], c["bias"]), (capi.OUT_F32, c["scale"], c["bias"]))
        new = [gpu_ctx.conv2d(d, c["x"], c["w"], s, b, ok) for ok, s, b in outs]
        with _GroupedOff(gpu_ctx.L):
            _named(gpu_ctx, d, IM2COL)
            old = [gpu_ctx.conv2d(d, c["x"], c["w"], s, b, ok) for ok, s, b in outs]
        _named(gpu_ctx, d)
        for a, b in zip(new, old):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("cin,cg", [(32, 4), (64, 8), (96, 16), (128, 32)])
def test_device_packer_equals_the_host_restatement(gpu_ctx, pkg, cin, cg):
    capi, C = pkg.capi, ctypes
    d = _desc(capi, _shape(1, cin, 7, 7, cg, P1, 1))
    _named(gpu_ctx, d)
    w = np.random.default_rng(cin).integers(-128, 128, (cin, cg, 3, 3)).astype(np.int8)
    nbytes = gpu_ctx.L.plhip_conv_packed_weight_bytes(C.byref(d))
    assert nbytes == cin // 32 * 9 * 1024
    dw, dwp = gpu_ctx.to_device(w), gpu_ctx.malloc(nbytes)
    gpu_ctx.check(gpu_ctx.L.plhip_pack_conv_weights(gpu_ctx.h, C.byref(d), dw, dwp), "pack")
    got = gpu_ctx.to_host(dwp, (cin // 32, 9, 64, 16), np.int8)
    gpu_ctx.free(dw), gpu_ctx.free(dwp)
    assert np.array_equal(got, pack_ref(w, cin, cg))
