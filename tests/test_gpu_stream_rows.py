"""GPU: the streaming fused depthwise3x3 -> pointwise1x1 kernel (fused_dwpw_stream.hip) on its six shapes, four of which take
their input rows through the wave-private LDS stage (StreamShape::ROWS, stream_rows.h), against the oracle's two-stage
computation: int32 accumulators and int8 output bit-exact, fp32 within the fused test's tolerance.  Inputs that make a
misplaced byte visible: +-127 on every border row and column, depthwise filters one-hot by channel % 9 (every tap alone: a byte
from across a row boundary, from a pad, or from the row above / below the image changes an accumulator), random filters too.
n = 1: the first plane is the last one (both ends of the tensor in one launch, grid rounded up to 8 with idle blocks); n = 3:
ragged XCD shares."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# c, h (= w), stride, m: the kernel's shapes (dw_plan.h kStreamShapes), the smallest its whitelist admits
SHAPES = {
    "112s1": (32, 112, 1, 64),
    "56s1": (128, 56, 1, 128),
    "28s1": (256, 28, 1, 256),   # register path
    "56s2": (64, 112, 2, 128),
    "28s2": (128, 56, 2, 256),
    "14s2": (256, 28, 2, 512),   # register path
}
RELU, RELU6, LEAKY = 1, 2, 4

CASES = [
    # shape, n, one-hot filters, dw_act, pw_act, int8_out
    ("112s1", 1, True, RELU, RELU, True),
    ("112s1", 3, False, RELU6, RELU6, True),
    ("112s1", 1, True, LEAKY, 0, False),      # fp32, stride 1
    ("56s1", 1, True, RELU, RELU, True),
    ("56s1", 3, False, LEAKY, RELU, True),
    ("56s1", 1, True, LEAKY, LEAKY, True),
    ("28s1", 1, True, RELU, RELU, True),
    ("28s1", 3, False, RELU6, LEAKY, True),
    ("56s2", 1, True, RELU, RELU, True),
    ("56s2", 3, False, RELU6, RELU6, True),
    ("56s2", 1, True, LEAKY, RELU, False),    # fp32, stride 2
    ("28s2", 1, True, RELU, RELU, True),
    ("28s2", 3, False, LEAKY, RELU6, True),
    ("28s2", 1, True, LEAKY, 0, True),
    ("28s2", 3, True, RELU6, RELU, True),
    ("14s2", 1, True, RELU, RELU, True),
    ("14s2", 3, False, LEAKY, RELU6, True),
]


def _inputs(rng, n, c, h, onehot):
    x = rng.integers(-127, 128, (n, c, h, h)).astype(np.int8)
    sign = (1 - 2 * ((np.arange(c)[:, None] + np.arange(h)[None, :]) % 2)).astype(np.int8)  # [channel][position along the border]
    x[:, :, :, 0] = 127 * sign
    x[:, :, :, -1] = -127 * sign
    x[:, :, 0, :] = 127 * sign
    x[:, :, -1, :] = -127 * sign
    if onehot:
        w_dw = np.zeros((c, 9), np.int8)
        w_dw[np.arange(c), np.arange(c) % 9] = 127
        w_dw = w_dw.reshape(c, 1, 3, 3)
    else:
        w_dw = rng.integers(-127, 128, (c, 1, 3, 3)).astype(np.int8)
    return x, w_dw


@pytest.mark.parametrize("shape,n,onehot,dw_act,pw_act,int8_out", CASES)
def test_stream_shapes_match_the_two_stage_oracle(gpu_ctx, pkg, plref, shape, n, onehot, dw_act, pw_act, int8_out):
    capi, ctx = pkg.capi, gpu_ctx
    c, h, stride, m = SHAPES[shape]
    rng = np.random.default_rng(1000 + 17 * n + len(shape) + dw_act)
    x, w_dw = _inputs(rng, n, c, h, onehot)
    w_pw = rng.integers(-127, 128, (m, c, 1, 1)).astype(np.int8)
    dw_alpha = 6.0 if dw_act == RELU6 else (0.2 if dw_act == LEAKY else 0.0)
    pw_alpha = 6.0 if pw_act == RELU6 else 0.3
    b_pw = rng.uniform(-1, 1, m).astype(np.float32)
    ws_pw = ((1 + np.arange(m) % 5) / 127.0 / 4.0).astype(np.float32)
    in_s = 1 / 127.0
    if onehot:  # the depthwise output is the input byte under the channel's tap (after the activation): nothing is rounded away
        b_dw = np.zeros(c, np.float32)
        ws_dw = np.full(c, 1 / 127.0, np.float32)
        mid_s = 1 / 127.0 if dw_act != RELU6 else dw_alpha / 127.0
    else:
        b_dw = rng.uniform(-1, 1, c).astype(np.float32)
        ws_dw = ((1 + np.arange(c) % 7) / 127.0 / 4.0).astype(np.float32)
        mid_s = 9 / 127.0 if dw_act != RELU6 else dw_alpha / 127.0
    out_s = c / 127.0 / 8 if pw_act != RELU6 else pw_alpha / 127.0
    pad = (1, 1, 1, 1)
    sd = plref.shape(n, c, h, h, c, 3, 3, pad, (stride, stride), (1, 1), c)
    oh, ow = plref.out_dims(sd)
    s1, b1, a1 = plref.fold_scales(1, in_s, ws_dw, mid_s, b_dw, c, dw_act, dw_alpha)
    d_ref, _ = plref.conv2d(sd, x, w_dw, b_dw, in_s, ws_dw, mid_s, dw_act, dw_alpha, True)
    sp = plref.shape(n, c, oh, ow, m, 1, 1, (0, 0, 0, 0), (1, 1), (1, 1), 1)
    y_ref, acc_ref = plref.conv2d(sp, d_ref, w_pw, b_pw, mid_s, ws_pw, out_s, pw_act, pw_alpha, int8_out)
    s2, b2, a2 = plref.fold_scales(int(int8_out), mid_s, ws_pw, out_s, b_pw, m, pw_act, pw_alpha)
    d_dw = capi.conv_desc(n, c, h, h, c, 3, 3, pad, (stride, stride), (1, 1), c, dw_act, a1)
    for kind in (capi.OUT_I32, capi.OUT_I8 if int8_out else capi.OUT_F32):
        assert ctx.L.plhip_dwpw_fused_supported(ctypes.byref(d_dw), m, kind) == 1, "the shape left the fused path"
    acc = ctx.dwpw_fused(d_dw, x, w_dw, s1, b1, w_pw, None, None, pw_act, a2, capi.OUT_I32)
    assert np.array_equal(acc, acc_ref), "fused int32 accumulators differ at %d places" % np.count_nonzero(acc != acc_ref)
    y = ctx.dwpw_fused(d_dw, x, w_dw, s1, b1, w_pw, s2, b2, pw_act, a2, capi.OUT_I8 if int8_out else capi.OUT_F32)
    if int8_out:
        assert np.array_equal(y, y_ref), "fused int8 output differs"
    else:
        np.testing.assert_allclose(y, y_ref, rtol=1e-5, atol=1e-6)
