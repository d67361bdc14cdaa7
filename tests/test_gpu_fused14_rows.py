"""GPU: the 14 x 14 fused depthwise -> pointwise kernel (fused_dwpw_i8.hip) after its input rows moved through a wave-private
LDS stage (int8 output) and its unused work was peeled off (every output kind).

Through the C ABI as test_gpu_fused_weight_ring.py does it: ctx.dwpw_fused against ctx.conv2d twice (the depthwise kernel, then
the 1x1 conv kernel) bit for bit, the smallest batch also against the two-stage oracle (test_gpu_fused._case).  Every case is a
14 x 14 plane."""
import ctypes

import numpy as np
import pytest

from test_gpu_fused import _case
from test_gpu_fused_weight_ring import _acc_of, _bits_equal, _fused, _operands, _two_kernels

pytestmark = pytest.mark.gpu

PAD = (1, 1, 1, 1)
HW = 14


@pytest.mark.parametrize("m", [256, 512])
@pytest.mark.parametrize("c", [128, 256, 512])
def test_every_form_matches_the_two_kernels(gpu_ctx, pkg, plref, c, m):
    """1, 2 and 4 rounds (C = 128: the first consuming round is the last one) x one and two m tiles per wave; batches 1, 3 and 9
    (2 / 6 / 18 tiles: the XCD remap's round-up blocks run and leave); relu6 on both stages and no activation; int8 (the staged
    rows), int32 and fp32 outputs (the rows straight from global memory) bit for bit.  Batch 1 also against the oracle."""
    capi = pkg.capi
    rng = np.random.default_rng(1400 + c + m)
    for act in (2, 0):
        for int8_out in (True, False):
            assert _case(gpu_ctx, capi, plref, rng, 1, c, HW, HW, 1, PAD, m, act, act, int8_out, pw_alpha=6.0, dw_alpha=6.0 if act == 2 else 0.0)
        for n in (1, 3, 9):
            what = "%d -> %d batch %d act %d" % (c, m, n, act)
            o = _operands(plref, rng, n, c, HW, m, act, act)
            d_dw, _, want = _two_kernels(gpu_ctx, capi, o, n, c, HW, 1, m, act, act, ("i32", "i8", "f32"))
            for kind in ("i32", "i8", "f32"):
                assert gpu_ctx.L.plhip_dwpw_fused_supported(ctypes.byref(d_dw), m, capi.OUT_I8 if kind == "i8" else capi.OUT_F32) == 1, what
                _bits_equal(_fused(gpu_ctx, capi, o, d_dw, act, kind), want[kind], "%s %s" % (what, kind))


def _leak_patterns(n, c):
    """(name, boolean mask of the nonzero input bytes): one set at a time."""
    def planes():
        return np.zeros((n * c, HW, HW), bool)
    k = planes()
    k[:, :, 0:2] = True
    yield "(a) columns 0-1 of every row", k
    k = planes()
    k[:, :, 12:14] = True
    yield "(b) columns 12-13 of every row", k
    k = planes()
    k[:, 6:8, :] = True
    yield "(c) rows 6-7: the seam and both halo rows", k
    k = planes()
    for b in range(n):
        for ch in (0, 15, 16, 127):  # task and round borders
            p = b * c + ch
            k[p, 13, :] = True
            if p + 1 < n * c:
                k[p + 1, 0, :] = True
    yield "(d) row 13 of channel c, row 0 of channel c + 1", k
    k = planes()
    for b in range(n - 1):
        k[(b + 1) * c - 1, 13, :] = True
        k[(b + 1) * c, 0, :] = True
    k[n * c - 1, 13, :] = True  # the tensor's very last row
    yield "(e) last row of image b, first row of image b + 1, the tensor's last row", k


def test_nothing_leaks_between_rows_halves_channels_and_images(gpu_ctx, pkg, plref):
    """C = 128, every depthwise weight 1, the depthwise stage requantises by 1 / 9 without an activation (|sum| <= 9 * 127: no
    saturation, one leaked byte of 127 moves its output by 14), inputs zero except one set of bytes at +127 and at -127.
    A row piece is fetched with one byte of each neighbouring row (of the next channel, the next image), the halves of a plane
    share two rows, and the slot of the row outside the image is never written: none of it may reach an output.
    int32 output (a leaked byte shows as itself and is not lost in saturation; the rows straight from global memory) exactly as
    the two kernels', and int8 output (the staged rows) through a pointwise stage that copies channel k % 128 to output k."""
    capi = pkg.capi
    n, c, m = 3, 128, 256
    rng = np.random.default_rng(1414)
    o = {"w_dw": np.ones((c, 1, 3, 3), np.int8),
         "w_pw": rng.integers(-127, 128, (m, c, 1, 1)).astype(np.int8),
         "s1": np.full(c, 1.0 / 9.0, np.float32), "b1": np.zeros(c, np.float32), "a1": 0.0,
         "i8": (np.ones(m, np.float32), np.zeros(m, np.float32), 0.0)}
    o["f32"] = o["i8"]
    copy = np.zeros((m, c, 1, 1), np.int8)
    copy[np.arange(m), np.arange(m) % c] = 1
    d_pw = capi.conv_desc(n, c, HW, HW, m, 1, 1, act=0, alpha=0.0)
    for name, k in _leak_patterns(n, c):
        for v in (127, -127):
            what = "%s at %d" % (name, v)
            o["x"] = np.where(k, v, 0).astype(np.int8).reshape(n, c, HW, HW)
            d_dw, mid, want = _two_kernels(gpu_ctx, capi, o, n, c, HW, 1, m, 0, 0, ("i32",))
            _bits_equal(_fused(gpu_ctx, capi, o, d_dw, 0, "i32"), want["i32"], what + " int32")
            want8 = gpu_ctx.conv2d(d_pw, mid, copy, o["i8"][0], o["i8"][1], capi.OUT_I8)
            _bits_equal(want8, np.concatenate([mid, mid], axis=1), what + ": the copying 1x1 conv")
            _bits_equal(_fused(gpu_ctx, capi, o, d_dw, 0, "i8", w_pw=copy), want8, what + " int8")


@pytest.mark.parametrize("c", [128, 512])
def test_first_and_last_k_step_alone(gpu_ctx, pkg, plref, c):
    """Batch 1, int8 output, pointwise weights zero outside one K-step (32 input channels), as
    test_one_k_step_of_weights_per_launch does it: the first K-step is the one multiplied into the constant 0, the last one
    belongs to the round that requests no next task and is multiplied from the fragments nobody fetches again.  Against the numpy
    accumulators through the oracle's epilogue, and against the two kernels."""
    capi = pkg.capi
    rng = np.random.default_rng(1430 + c)
    for m in (256, 512):
        o = _operands(plref, rng, 1, c, HW, m, 1, 1)
        d_dw, mid, _ = _two_kernels(gpu_ctx, capi, o, 1, c, HW, 1, m, 1, 1, ())
        d_pw = capi.conv_desc(1, c, HW, HW, m, 1, 1, act=1, alpha=o["i8"][2])
        for ks in (0, c // 32 - 1):
            what = "%d -> %d K-step %d" % (c, m, ks)
            k = np.zeros((m, c, 1, 1), bool)
            k[:, 32 * ks:32 * ks + 32] = True
            w = np.where(k, o["w_pw"], 0).astype(np.int8)
            got = _fused(gpu_ctx, capi, o, d_dw, 1, "i8", w_pw=w)
            _bits_equal(got, plref.epilogue(_acc_of(mid, w), o["i8"][0], o["i8"][1], 1, o["i8"][2], True), what + " against numpy")
            _bits_equal(got, gpu_ctx.conv2d(d_pw, mid, w, o["i8"][0], o["i8"][1], capi.OUT_I8), what + " against the two kernels")


def test_batch_128_matches_the_two_kernels(gpu_ctx, pkg, plref):
    """The benchmark's own grid: 512 -> 512, relu6 on both stages, 256 tiles = one wave of blocks; int8 output bit for bit."""
    capi = pkg.capi
    n, c, m = 128, 512, 512
    rng = np.random.default_rng(1450)
    o = _operands(plref, rng, n, c, HW, m, 2, 2)
    d_dw, _, want = _two_kernels(gpu_ctx, capi, o, n, c, HW, 1, m, 2, 2, ("i8",))
    _bits_equal(_fused(gpu_ctx, capi, o, d_dw, 2, "i8"), want["i8"], "512 -> 512 batch 128 int8")
