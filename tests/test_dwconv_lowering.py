"""Host logic of fusion G (GraphBuilder::set_fuse_dwconv, plhip_dw_conv1x1_fused_supported), checked on the CPU: the opt-in
rewrite of depthwise_conv2d[int8_out] -> conv2d 1x1 with the conv's fused tail into one instruction, and the envelope of the
fused kernel's predicate."""
import ctypes
import importlib
import re

import pytest

# MobileNetV2-224's 17 block pairs: (C, input plane, stride, M)
V2_PAIRS = [(32, 112, 1, 16), (96, 112, 2, 24), (144, 56, 1, 24), (144, 56, 2, 32), (192, 28, 1, 32), (192, 28, 1, 32),
            (192, 28, 2, 64), (384, 14, 1, 64), (384, 14, 1, 64), (384, 14, 1, 64), (384, 14, 1, 96), (576, 14, 1, 96),
            (576, 14, 1, 96), (576, 14, 2, 160), (960, 7, 1, 160), (960, 7, 1, 160), (960, 7, 1, 320)]


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


def _plan(lite, wl, net, batch=1, fuse=True, fuse_dwconv=None):
    p = lite.Predictor(planner=True)
    try:
        wl.emit_graph(p, net, batch, fuse=fuse, fuse_dwconv=fuse_dwconv)
        return p.graph_plan()
    finally:
        p.close()


def _nets(wl):
    return {"v1_224": wl.mobilenet_v1_net(), "v1_192": wl.mobilenet_v1_net(res=192), "v2_224": wl.mobilenet_v2_net(),
            "r50_64": wl.resnet50_net(res=64)}


def test_unset_equals_off(lite, wl):
    """With G unset every program is the one G off gives (the switch defaults to off)."""
    for name, net in _nets(wl).items():
        for batch in (1, 128):
            assert _plan(lite, wl, net, batch) == _plan(lite, wl, net, batch, fuse_dwconv=False), name


def test_mobilenet_v2_with_fusion_g(lite, wl):
    net = wl.mobilenet_v2_net()
    for batch in (1, 128):
        off = _plan(lite, wl, net, batch, fuse_dwconv=False)
        on = _plan(lite, wl, net, batch, fuse_dwconv=True)
        assert len(off) == 58 and len(on) == 41
        g = [l for l in on if "+conv1x1=" in l]
        assert len(g) == 17 and all(l.startswith("depthwise_conv2d/int8_out ") for l in g)
        assert [l.split(" via=")[1].split(" ")[0] for l in g] == ["b%d_dw" % i for i in range(1, 18)]
        assert not any("+pw=" in l for l in on)
        # no instruction reads a depthwise result any more
        for l in on:
            ins = l.split(" in=")[1].split(" ")[0].split(",")
            assert not any(re.fullmatch(r"b\d+_dw", v) for v in ins), l
        # b1 / b17 are int8_out; the other 15 carry the 1x1 line's own tail fields, as its unfused line had them
        unfused = {l.split(" in=")[1].split(" ")[0]: l for l in off if l.startswith("conv2d/")}
        for b, l in enumerate(g, start=1):
            kind = "int8_out" if b in (1, 17) else "fp32_out"
            assert " +conv1x1=conv2d/%s via=b%d_dw" % (kind, b) in l, l
            pw = unfused["b%d_dw" % b]
            assert pw.startswith("conv2d/" + kind)
            assert l.split(" out=")[1].split(" ")[0] == pw.split(" out=")[1].split(" ")[0]
            tail = pw.split(" out=")[1].split(" ", 1)[1]  # oscale / +add / +calib / -f32 of the unfused 1x1 line
            assert l.endswith(" via=b%d_dw " % b + tail), (l, pw)
            if kind == "fp32_out":
                assert "+calib=" in l
        assert sum("+add=" in l for l in g) == 10 and sum(" -f32" in l for l in g) == sum(" -f32" in l for l in off)
        # everything else is untouched, in order
        rest_on = [l for l in on if "+conv1x1=" not in l]
        g_outs = {l.split(" out=")[1].split(" ")[0] for l in g}
        rest_off = [l for l in off if not l.startswith("depthwise_conv2d/") and l.split(" out=")[1].split(" ")[0] not in g_outs]
        assert rest_on == rest_off


def test_mobilenet_v1_with_fusion_g(lite, wl):
    v1 = wl.mobilenet_v1_net()
    # at 224 fusion D takes all 13 pairs first: G finds nothing left
    assert _plan(lite, wl, v1, 2, fuse_dwconv=True) == _plan(lite, wl, v1, 2, fuse_dwconv=False)
    v192 = wl.mobilenet_v1_net(res=192)
    on, off = _plan(lite, wl, v192, 2, fuse_dwconv=True), _plan(lite, wl, v192, 2, fuse_dwconv=False)
    g = [l for l in on if "+conv1x1=" in l]
    assert len(g) == 13 and len(on) == len(off) - 13 and not any("+pw=" in l for l in on)
    assert [l.split(" via=")[1].split(" ")[0] for l in g] == ["dw%d" % i for i in range(2, 15)]
    assert sum(l.startswith("pool2d/") for l in on) == 1  # the pool stays its own instruction
    # set_fuse(false) with G on is the reference program
    assert _plan(lite, wl, v192, 2, fuse=False, fuse_dwconv=True) == _plan(lite, wl, v192, 2, fuse=False, fuse_dwconv=False)
    assert not any("+conv1x1=" in l for l in _plan(lite, wl, v192, 2, fuse=False, fuse_dwconv=True))


def test_resnet50_untouched_by_fusion_g(lite, wl):
    net = wl.resnet50_net(res=64)
    assert _plan(lite, wl, net, 2, fuse_dwconv=True) == _plan(lite, wl, net, 2, fuse_dwconv=False)


def _dw(capi, n, c, h, k=3, pad=1, stride=1, dil=1, mult=1, act=0):
    return capi.conv_desc(n, c, h, h, c * mult, k, k, (pad,) * 4, (stride, stride), (dil, dil), c, act, 0.0)


def test_predicate_envelope(pkg):
    capi = pkg.capi
    L = capi.load()
    sup = lambda d, m, out, tail: L.plhip_dw_conv1x1_fused_supported(ctypes.byref(d), m, out, int(tail))  # noqa: E731
    for (c, hw, s, m) in V2_PAIRS:
        for n in (1, 2, 128, 1024):
            d = _dw(capi, n, c, hw, stride=s)
            for tail in (False, True):
                assert sup(d, m, capi.OUT_F32, tail) == 1, (n, c, hw, s, m, tail)
            assert sup(d, m, capi.OUT_I8, False) == 1 and sup(d, m, capi.OUT_I32, False) == 1
    # other shapes inside the envelope: odd planes, asymmetric / zero paddings, every activation, C = 16, M = 8 .. 1024
    assert sup(capi.conv_desc(2, 16, 9, 13, 16, 3, 3, (0, 1, 1, 0), (2, 2), (1, 1), 16, 1, 0.0), 8, capi.OUT_F32, True) == 1
    assert sup(_dw(capi, 1, 1024, 7), 1024, capi.OUT_I8, False) == 1
    for act in (0, 1, 2, 4):
        assert sup(_dw(capi, 1, 64, 10, pad=0, act=act), 72, capi.OUT_F32, False) == 1
    # refused
    assert sup(_dw(capi, 2, 32, 8, k=5, pad=2), 16, capi.OUT_F32, False) == 0             # 5x5
    assert sup(_dw(capi, 2, 32, 8, pad=2, dil=2), 16, capi.OUT_F32, False) == 0           # dilation 2
    assert sup(_dw(capi, 2, 24, 8), 16, capi.OUT_F32, False) == 0                         # C = 24
    assert sup(_dw(capi, 2, 32, 8, mult=2), 16, capi.OUT_F32, False) == 0                 # channel multiplier 2
    assert sup(_dw(capi, 2, 32, 8), 33, capi.OUT_F32, False) == 0                         # M = 33
    assert sup(_dw(capi, 2, 32, 8), 16, capi.OUT_I8, True) == 0                           # a tail with int8 output
    assert sup(_dw(capi, 2, 32, 8), 16, capi.OUT_F32_GAP, False) == 0                     # the plane average
    assert sup(_dw(capi, 2, 32, 8, pad=2), 16, capi.OUT_F32, False) == 0                  # padding 2
    assert sup(_dw(capi, 2, 32, 8, stride=3), 16, capi.OUT_F32, False) == 0               # stride 3
    assert sup(_dw(capi, 2, 2048, 8), 16, capi.OUT_F32, False) == 0                       # C > 1024
    assert sup(_dw(capi, 2, 32, 8), 1032, capi.OUT_F32, False) == 0                       # M > 1024
    assert sup(_dw(capi, 4096, 256, 56), 256, capi.OUT_F32, False) == 0                   # element offsets past 2^31
