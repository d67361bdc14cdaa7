"""GPU: the pointwise-weight ring of the fused depthwise -> pointwise kernels (fused_dwpw_stream.hip on the 14-wide plane,
fused_dwpw_small.hip on the 7 x 7 planes): the forms whose ring holds four K-steps / a whole pass of weight fragments.

Every output kind and batch sizes whose tile counts are no multiple of 8 against the two-kernel path (depthwise kernel, then
the 1x1 conv kernel) bit for bit, the smallest batch against the two-stage oracle as test_gpu_fused.py does it, and launches
whose pointwise weights are zero outside one K-step: a fragment multiplied from the wrong slot of the ring, or one K-step late,
meets activations of other channels and changes the accumulators of that launch."""
import ctypes

import numpy as np
import pytest

from test_gpu_fused import _case

pytestmark = pytest.mark.gpu

# c, input plane, depthwise stride, m: 256 -> 512 s2 @28 (streaming kernel, two passes over M, a whole pass of weights in
# registers), 512 -> 1024 s2 @14 and 1024 -> 1024 @7 (7 x 7 kernel, four m tiles per wave, four ring slots)
SHAPES = [(256, 28, 2, 512), (512, 14, 2, 1024), (1024, 7, 1, 1024)]
IDS = ["256-512s2@28", "512-1024s2@14", "1024-1024@7"]
PAD = (1, 1, 1, 1)


def _bits_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = g != w
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %s want %s" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:6], want[bad][:6])


def _operands(plref, rng, n, c, hw, m, dw_act, pw_act):
    """Operands and folded scales of one pair, the scales of test_gpu_fused._case."""
    o = {"x": rng.integers(-127, 128, (n, c, hw, hw)).astype(np.int8),
         "w_dw": rng.integers(-127, 128, (c, 1, 3, 3)).astype(np.int8),
         "w_pw": rng.integers(-127, 128, (m, c, 1, 1)).astype(np.int8)}
    b_dw = rng.uniform(-1, 1, c).astype(np.float32)
    b_pw = rng.uniform(-1, 1, m).astype(np.float32)
    ws_dw = ((1 + np.arange(c) % 7) / 127.0 / 4.0).astype(np.float32)
    ws_pw = ((1 + np.arange(m) % 5) / 127.0 / 4.0).astype(np.float32)
    dw_alpha, pw_alpha = (6.0 if dw_act == 2 else 0.0), (6.0 if pw_act == 2 else 0.0)
    mid_s = 9 / 127.0 if dw_act != 2 else dw_alpha / 127.0
    out_s = c / 127.0 / 8 if pw_act != 2 else pw_alpha / 127.0
    o["s1"], o["b1"], o["a1"] = plref.fold_scales(1, 1 / 127.0, ws_dw, mid_s, b_dw, c, dw_act, dw_alpha)
    o["i8"] = plref.fold_scales(1, mid_s, ws_pw, out_s, b_pw, m, pw_act, pw_alpha)
    o["f32"] = plref.fold_scales(0, mid_s, ws_pw, out_s, b_pw, m, pw_act, pw_alpha)
    return o


def _two_kernels(ctx, capi, o, n, c, hw, st, m, dw_act, pw_act, kinds):
    """The pair as two launches: the int8 tensor between them and the pointwise outputs of `kinds`."""
    d_dw = capi.conv_desc(n, c, hw, hw, c, 3, 3, PAD, (st, st), (1, 1), c, dw_act, o["a1"])
    mid = ctx.conv2d(d_dw, o["x"], o["w_dw"], o["s1"], o["b1"], capi.OUT_I8, depthwise=True)
    out = {}
    for kind in kinds:
        sc, bi, al = (None, None, o["i8"][2]) if kind == "i32" else o[kind]
        d_pw = capi.conv_desc(n, c, hw // st, hw // st, m, 1, 1, act=pw_act, alpha=al)
        out[kind] = ctx.conv2d(d_pw, mid, o["w_pw"], sc, bi, {"i32": capi.OUT_I32, "i8": capi.OUT_I8, "f32": capi.OUT_F32}[kind])
    return d_dw, mid, out


def _fused(ctx, capi, o, d_dw, pw_act, kind, w_pw=None):
    sc, bi, al = (None, None, o["i8"][2]) if kind == "i32" else o["f32" if kind == "gap" else kind]
    ok = {"i32": capi.OUT_I32, "i8": capi.OUT_I8, "f32": capi.OUT_F32, "gap": capi.OUT_F32_GAP}[kind]
    return ctx.dwpw_fused(d_dw, o["x"], o["w_dw"], o["s1"], o["b1"], o["w_pw"] if w_pw is None else w_pw, sc, bi, pw_act, al, ok)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_output_kind_matches_the_two_kernels(gpu_ctx, pkg, plref, shape):
    """Batches 1, 3 and 9 (2 / 6 / 18 tiles of the 14-wide plane, 1 / 3 / 9 blocks of the 7 x 7 planes: the XCD remap's
    round-up blocks run and leave), relu6 on both stages and no activation at all; int32, int8 and fp32 outputs bit for bit
    against the two kernels; the pooled fp32 output of the last pair against the average of the two kernels' fp32 output
    within 1e-5 (the bound of test_fused_pair_with_the_global_average_as_output: the sum's order differs, the values summed
    are the bit-identical fp32 outputs).  Batch 1 also against the two-stage oracle."""
    capi = pkg.capi
    c, hw, st, m = shape
    rng = np.random.default_rng(410 + c)
    for act in (2, 0):
        for int8_out in (True, False):
            assert _case(gpu_ctx, capi, plref, rng, 1, c, hw, hw, st, PAD, m, act, act, int8_out, pw_alpha=6.0, dw_alpha=6.0 if act == 2 else 0.0)
        for n in (1, 3, 9):
            what = "%s batch %d act %d" % (shape, n, act)
            o = _operands(plref, rng, n, c, hw, m, act, act)
            d_dw, _, want = _two_kernels(gpu_ctx, capi, o, n, c, hw, st, m, act, act, ("i32", "i8", "f32"))
            for kind in ("i32", "i8", "f32"):
                assert gpu_ctx.L.plhip_dwpw_fused_supported(ctypes.byref(d_dw), m, capi.OUT_I8 if kind == "i8" else capi.OUT_F32) == 1, what
                _bits_equal(_fused(gpu_ctx, capi, o, d_dw, act, kind), want[kind], "%s %s" % (what, kind))
            if shape == SHAPES[-1]:
                pooled = want["f32"].astype(np.float64).mean(axis=(2, 3)).astype(np.float32).reshape(n, m, 1, 1)
                np.testing.assert_allclose(_fused(gpu_ctx, capi, o, d_dw, act, "gap"), pooled, rtol=1e-5, atol=1e-6, err_msg=what + " pooled")


def _acc_of(mid, w_pw):
    """int32 accumulators of the 1x1 conv in numpy: |sum| <= 1024 * 128 * 128 < 2^53, exact in float64."""
    n, c, oh, ow = mid.shape
    acc = np.matmul(w_pw.reshape(-1, c).astype(np.float64), mid.reshape(n, c, oh * ow).astype(np.float64))
    return acc.astype(np.int32).reshape(n, -1, oh, ow)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_k_step_of_weights_per_launch(gpu_ctx, pkg, plref, shape):
    """Batch 1.  One launch per K-step ks (32 input channels) with pointwise weights that are zero outside it: the int32
    accumulators must be that K-step's product alone.  Then the ring's edges: the last K-step of pass 0 with the first of
    pass 1 (the 14-wide form: pass p owns output channels [256 p, 256 p + 256)), and the last four K-steps (the 7 x 7 kernel's
    last turn of its four slots)."""
    capi = pkg.capi
    c, hw, st, m = shape
    ks_n = c // 32
    rng = np.random.default_rng(520 + c)
    o = _operands(plref, rng, 1, c, hw, m, 1, 1)
    d_dw, mid, want = _two_kernels(gpu_ctx, capi, o, 1, c, hw, st, m, 1, 1, ("i32",))
    _bits_equal(_acc_of(mid, o["w_pw"]), want["i32"], "%s: numpy product against the 1x1 conv kernel" % (shape,))
    masks = []
    for ks in range(ks_n):
        k = np.zeros((m, c), bool)
        k[:, 32 * ks:32 * ks + 32] = True
        masks.append(("K-step %d" % ks, k))
    k = np.zeros((m, c), bool)
    if shape == SHAPES[0]:
        k[:m // 2, c - 32:] = True
        k[m // 2:, :32] = True
        masks.append(("pass hand-over", k))
    else:
        k[:, c - 4 * 32:] = True
        masks.append(("last four K-steps", k))
    for name, k in masks:
        w = np.where(k.reshape(m, c, 1, 1), o["w_pw"], 0).astype(np.int8)
        _bits_equal(_fused(gpu_ctx, capi, o, d_dw, 1, "i32", w_pw=w), _acc_of(mid, w), "%s %s" % (shape, name))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_batch_128_matches_the_two_kernels(gpu_ctx, pkg, plref, shape):
    """The benchmark's batch: one full wave of blocks (256 tiles of the 14-wide plane, 128 blocks of the 7 x 7 planes); int8
    output bit for bit against the two kernels."""
    capi = pkg.capi
    c, hw, st, m = shape
    rng = np.random.default_rng(630 + c)
    o = _operands(plref, rng, 128, c, hw, m, 1, 1)
    d_dw, _, want = _two_kernels(gpu_ctx, capi, o, 128, c, hw, st, m, 1, 1, ("i8",))
    _bits_equal(_fused(gpu_ctx, capi, o, d_dw, 1, "i8"), want["i8"], "%s batch 128 int8" % (shape,))
