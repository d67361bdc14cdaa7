"""GPU: every int8 kernel route on its value edges (operands from edge_cases.py), against the oracle.

Folded per-channel scales 2^-e and quarter biases go straight through the C ABI, so the results sit on exact ties of both signs,
on +-127.5, past both saturation bounds, on a relu6 bound that is an integer, a half-integer or above 127, and on leaky ties
after the alpha multiply; a maximum-magnitude case per route adds +-127 / -128 operands (|acc| > 2^24 where K allows).
int32 accumulators, int8 outputs and fp32 outputs are compared bit for bit: both sides compute one fmaf of the same operands and
the same activation.  The set of routes that ran is checked against the route table, so a dispatch change cannot drop one."""
import ctypes

import numpy as np
import pytest

import edge_cases as E

pytestmark = pytest.mark.gpu


def _eq(got, want, what):
    assert got.dtype == want.dtype, what
    if got.dtype == np.float32:  # bit for bit (the same fmaf on both sides); -0.0 and 0.0 differ here
        bad = got.view(np.uint32) != want.view(np.uint32)
    else:
        bad = got != want
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %s want %s" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:6], want[bad][:6])


def _desc(capi, c, route, act, alpha):
    n, _, h, w, cout, kh, kw, pads, st, dl, g = route["shape"]
    cin = c["cin"]
    if route["kind"] == "dw":
        g, cout = cin, cin
    return capi.conv_desc(n, cin, h, w, cout, kh, kw, pads, (st, st), (dl, dl), g, act, alpha)


def _ran(capi, route, c):
    """The kernels the route's launches reach for every output kind under the knobs in force (edge_cases.kernel_of: the
    library's own launch plan for the GEMM routes)."""
    cin = c["cin"] if "cin" in c else c["x"].shape[1]
    return {E.kernel_of(capi, route, cin, out) for out in ("i32", "i8", "f32")}


def _run(ctx, capi, route, c, act, alpha):
    """Runs one case on every output kind of the route."""
    kind, what = route["kind"], "%s act %d alpha %g" % (route["name"], act, alpha)
    outs = ((capi.OUT_I32, "acc"), (capi.OUT_I8, "ref_i8"), (capi.OUT_F32, "ref_f32"))
    if kind in ("conv", "dw"):
        d = _desc(capi, c, route, act, alpha)
        if kind == "conv":
            assert ctx.L.plhip_conv_impl_name(ctypes.byref(d)).decode() == route["impl"], what
        for ok, key in outs:
            sc, bi = (None, None) if ok == capi.OUT_I32 else (c["scale"], c["bias"])
            _eq(ctx.conv2d(d, c["x"], c["w"], sc, bi, ok, depthwise=kind == "dw"), c[key], "%s %s" % (what, key))
    elif kind == "calib":
        d = _desc(capi, c, route, act, alpha)
        assert ctx.L.plhip_conv2d_calib_supported(ctypes.byref(d)) == 1
        for ok, key in outs:
            sc, bi = (None, None) if ok == capi.OUT_I32 else (c["scale"], c["bias"])
            _eq(ctx.conv2d_calib(d, c["xf"], c["calib"], c["w"], sc, bi, ok), c[key], "%s %s" % (what, key))
    elif kind == "image":
        d = _desc(capi, c, route, act, alpha)
        n, _, h, w = route["shape"][:4]
        img = capi.image_desc(n, h, w, capi.IMG_BGR, E.IMG_MEANS, E.IMG_SCALES)
        assert ctx.L.plhip_conv2d_image_supported(ctypes.byref(d), ctypes.byref(img)) == 1
        for ok, key in outs:
            sc, bi = (None, None) if ok == capi.OUT_I32 else (c["scale"], c["bias"])
            _eq(ctx.conv2d_image(d, img, c["src"], E.IMG_CALIB, c["w"], sc, bi, ok), c[key], "%s %s" % (what, key))
    elif kind in ("dwpw", "dwconv"):
        n, cin, h, w, _, _, _, pads, st, _, _ = route["shape"]
        d_dw = capi.conv_desc(n, cin, h, w, cin, 3, 3, pads, (st, st), (1, 1), cin, c["dw_act"], c["dw_alpha"])
        _eq(ctx.conv2d(d_dw, c["x"], c["w_dw"], c["s1"], c["b1"], capi.OUT_I8, depthwise=True), c["mid"], what + " dw stage")
        for ok, key in outs:
            sc, bi = (None, None) if ok == capi.OUT_I32 else (c["scale"], c["bias"])
            if kind == "dwpw":
                assert ctx.L.plhip_dwpw_fused_supported(ctypes.byref(d_dw), route["m"], ok) == 1, what
                y = ctx.dwpw_fused(d_dw, c["x"], c["w_dw"], c["s1"], c["b1"], c["w"], sc, bi, act, alpha, ok)
            else:
                assert ctx.L.plhip_dw_conv1x1_fused_supported(ctypes.byref(d_dw), route["m"], ok, 0) == 1, what
                y, _ = ctx.dw_conv1x1_fused(d_dw, c["x"], c["w_dw"], c["s1"], c["b1"], c["w"], sc, bi, act, alpha, ok)
            _eq(y, c[key], "%s %s" % (what, key))
    elif kind == "fc":
        relu = int(act == E.ACT_RELU)
        for ok, key in outs:
            sc, bi = (None, None) if ok == capi.OUT_I32 else (c["scale"], c["bias"])
            _eq(ctx.fc(c["x"], c["w"], sc, bi, relu, ok), c[key], "%s %s" % (what, key))
    elif kind == "tail":
        d = _desc(capi, c, route, act, alpha)
        assert ctx.L.plhip_conv_impl_name(ctypes.byref(d)).decode() == route["impl"], what
        yf, yq = ctx.conv2d_fused(d, c["x"], c["w"], c["scale"], c["bias"], c["res"], int(c["res_relu"]), c["calib"])
        _eq(yf, c["ref_z"], what + " fp32 sum")
        _eq(yq, c["ref_q"], what + " calib copy")
    else:
        raise AssertionError(kind)


@pytest.mark.parametrize("maxmag", [False, True], ids=["edges", "max_magnitude"])
def test_every_route_on_its_value_edges(gpu_ctx, pkg, plref, maxmag):
    capi = pkg.capi
    lib = capi.load()
    ran = set()
    for i, route in enumerate(E.ROUTES):
        acts = E.acts_of(route)
        if maxmag:  # no activation, and leaky where the route has it
            acts = acts[:1] if route["kind"] in ("fc", "tail") else (acts[0], (E.ACT_LEAKY, 0.375))
        with E.Knobs(lib, route["knobs"]):
            for j, (act, alpha) in enumerate(acts):
                c = E.make_case(plref, route, act, alpha, maxmag, E.case_seed(i, route, j, maxmag))
                _run(gpu_ctx, capi, route, c, act, alpha)
                k = _ran(capi, route, c)
                assert k == {E.kernel_for(route, out) for out in ("i32", "i8", "f32")}, (route["name"], k)  # the knob reached the kernel the route names
                ran |= k
    assert ran == {E.kernel_for(r, out) for r in E.ROUTES for out in ("i32", "i8", "f32")}, sorted(ran)
    print("kernels on their edges:", sorted(ran))


# ---- grid edges: batch sizes around the XCD-contiguous block map ----------------------------------------------------------
# (vb = (bid & 7) * per + (bid >> 3) with `vb >= nb` early returns, ragged shares and the launchers' magic-number divisions).
# Every image is distinct and every output buffer is filled with a poison byte before the launch, so an image written to the
# wrong place or not written at all cannot pass as the right one.
BATCH_ROUTES = {"dwpw_14x14": (1, 7, 8, 9, 17, 128, 129), "dwpw_7x7": (1, 7, 8, 9, 17, 128, 129),
                "stem_f32_calib": (1, 7, 8, 9, 17, 128, 129), "stem_u8_image": (1, 7, 8, 9, 17, 128, 129),
                "dwpw_stream_s2": (1, 7, 8, 9, 17), "dwpw_stream": (1, 7, 8, 9, 17), "stem7x7s2": (1, 7, 8, 9, 17),
                "direct3x3s2_mfma": (1, 7, 8, 9, 17), "dw3x3s1_direct": (1, 7, 8, 9, 17), "gemm_ring": (1, 7, 8, 9, 17),
                "gemm_wide_n4": (1, 7, 8, 9, 17), "dw_conv1x1_wide130": (1, 7, 8, 9, 17)}
POISON = 0xA5


class _Poisoned:
    """Every device buffer the context allocates is filled with POISON before use (inputs are then overwritten by their copy)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        ctx, plain = self.ctx, type(self.ctx).malloc

        def malloc(nbytes):
            p = plain(ctx, nbytes)
            ctx.check(ctx.L.plhip_memset(ctx.h, p, POISON, nbytes), "memset")
            return p
        ctx.malloc = malloc

    def __exit__(self, *a):
        del self.ctx.malloc


def _first(c, route, n):
    """The case's first n images (and the route at batch n)."""
    out = dict(c)
    for key in ("x", "xf", "src"):
        if key in c:
            out[key] = c[key][:n]
    return out, dict(route, shape=(n,) + tuple(route["shape"][1:]))


def _y(ctx, capi, route, c, act, alpha):
    kind = route["kind"]
    n, _, h, w = route["shape"][:4]
    d = _desc(capi, c, route, act, alpha)
    if kind == "conv":
        return ctx.conv2d(d, c["x"], c["w"], c["scale"], c["bias"], capi.OUT_I8)
    if kind == "dw":
        return ctx.conv2d(d, c["x"], c["w"], c["scale"], c["bias"], capi.OUT_I8, depthwise=True)
    if kind == "calib":
        return ctx.conv2d_calib(d, c["xf"], c["calib"], c["w"], c["scale"], c["bias"], capi.OUT_I8)
    if kind == "image":
        img = capi.image_desc(n, h, w, capi.IMG_BGR, E.IMG_MEANS, E.IMG_SCALES)
        return ctx.conv2d_image(d, img, c["src"], E.IMG_CALIB, c["w"], c["scale"], c["bias"], capi.OUT_I8)
    cin, pads, st = route["shape"][1], route["shape"][7], route["shape"][8]
    d_dw = capi.conv_desc(n, cin, h, w, cin, 3, 3, pads, (st, st), (1, 1), cin, c["dw_act"], c["dw_alpha"])
    if kind == "dwconv":
        return ctx.dw_conv1x1_fused(d_dw, c["x"], c["w_dw"], c["s1"], c["b1"], c["w"], c["scale"], c["bias"], act, alpha, capi.OUT_I8)[0]
    assert kind == "dwpw", kind
    return ctx.dwpw_fused(d_dw, c["x"], c["w_dw"], c["s1"], c["b1"], c["w"], c["scale"], c["bias"], act, alpha, capi.OUT_I8)


def test_batch_sweep_matches_single_images(gpu_ctx, pkg, plref):
    """Batch n in {1, 7, 8, 9, 17} (and 128 / 129 for the fused 14 x 14 and 7 x 7 kernels and the 3x3 stems) of max(n) distinct
    images: every image of every batch-n run equals the oracle, and so does the batch-1 run of the first, middle and last."""
    capi = pkg.capi
    lib = capi.load()
    byname = {r["name"]: r for r in E.ROUTES}
    for i, (name, ns) in enumerate(BATCH_ROUTES.items()):
        big = max(ns)
        route = dict(byname[name], shape=(big,) + tuple(byname[name]["shape"][1:]))
        act, alpha = E.ACTS[i % len(E.ACTS)]
        c = E.make_case(plref, route, act, alpha, False, 9000 + i)
        ref = c["ref_i8"]
        assert len({ref[b].tobytes() for b in range(big)}) == big, name  # distinct images, distinct outputs
        with E.Knobs(lib, route["knobs"]), _Poisoned(gpu_ctx):
            for n in ns:
                y = _y(gpu_ctx, capi, *reversed(_first(c, route, n)), act, alpha)
                for b in range(n):
                    _eq(y[b], ref[b], "%s n=%d image %d" % (name, n, b))
            for b in (0, big // 2, big - 1):
                cb = dict(c)
                for key in ("x", "xf", "src"):
                    if key in c:
                        cb[key] = c[key][b:b + 1]
                y1 = _y(gpu_ctx, capi, dict(route, shape=(1,) + tuple(route["shape"][1:])), cb, act, alpha)
                _eq(y1[0], ref[b], "%s batch-1 run of image %d" % (name, b))
