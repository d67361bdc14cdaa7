"""GPU: fusion G (plhip_dw_conv1x1_fused_int8) executing every regime of its launch plan, on the cases of dwconv_cases.py
(test_dwconv_cases.py proves on the host that each case is in the regime it names and that the operands reach their edges).

Every case: int32 accumulators and the int8 output equal the oracle's bit for bit; the fp32 output is within rtol 1e-5 of the
oracle and byte-identical to the two launches it replaces.  The cases with stated seeds also run the graph tail (calib copy
alone, residual sum with and without relu, the fp32 sum kept and dropped), outputs 1, 2, 3 elements off their alignment, and a
batch sweep of distinct images.  Every fused launch writes into allocations filled with 0xA5 whose margins must come back
untouched, so a value stored outside the tensor, or not stored at all, cannot pass."""
import ctypes

import numpy as np
import pytest

import dwconv_cases as D
import edge_cases as E

pytestmark = pytest.mark.gpu
POISON = 0xA5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = (_bits(got) != _bits(want)) if got.dtype == np.float32 else (got != want)
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %s want %s" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:6], want[bad][:6])


def _fused(ctx, capi, case, c, act, alpha, out, what, x=None, y_off=0, q_off=0, **tail):
    """One fused launch into poisoned, guarded outputs: (y, y_i8) after the margins of both were found untouched."""
    x = c["x"] if x is None else x
    d = D.desc_of(capi, case["shape"], c["dw_act"], c["dw_alpha"], n=x.shape[0])
    assert ctx.L.plhip_dw_conv1x1_fused_supported(ctypes.byref(d), case["shape"][6], out, int(bool(tail))) == 1, what
    sc, bi = (None, None) if out == capi.OUT_I32 else (c["scale"], c["bias"])
    y, yq, my, mq = ctx.dw_conv1x1_fused(d, x, c["w_dw"], c["s1"], c["b1"], c["w"], sc, bi, act, alpha, out,
                                         misalign=(case["x_off"], y_off, q_off), sentinel=POISON, **tail)
    for m, name in ((my, "y"), (mq, "y_i8")):
        assert m is None or (m == POISON).all(), "%s: %d bytes written outside %s" % (what, (m != POISON).sum(), name)
    return y, yq


def _two_launches(ctx, capi, case, c, act, alpha, x=None, **tail):
    """The launches the fused one replaces: depthwise (int8 out), then the 1x1 conv, with its tail when there is one."""
    x = c["x"] if x is None else x
    n, (oh, ow) = x.shape[0], c["mid"].shape[2:]
    mid = ctx.conv2d(D.desc_of(capi, case["shape"], c["dw_act"], c["dw_alpha"], n=n), x, c["w_dw"], c["s1"], c["b1"], capi.OUT_I8,
                     depthwise=True)
    d_pw = capi.conv_desc(n, case["shape"][1], oh, ow, case["shape"][6], 1, 1, act=act, alpha=alpha)
    if tail:
        return mid, ctx.conv2d_fused(d_pw, mid, c["w"], c["scale"], c["bias"], tail.get("residual"), tail.get("residual_relu", 0),
                                     tail.get("calib_scale"), tail.get("want_y", True))
    return mid, (ctx.conv2d(d_pw, mid, c["w"], c["scale"], c["bias"], capi.OUT_F32), None)


@pytest.mark.parametrize("group", D.GROUPS)
def test_every_regime_equals_the_oracle_and_the_two_launches(gpu_ctx, pkg, plref, group):
    capi = pkg.capi
    ran = 0
    for case in (c for c in D.CASES if c["group"] == group):
        for j, (act, alpha, _seed) in enumerate(D.acts_of(case)):
            c = D.reference(plref, case, j)
            what = "%s act %d alpha %g" % (case["name"], act, alpha)
            _eq(_fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_I32, what)[0], c["acc"], what + " int32 accumulators")
            _eq(_fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_I8, what)[0], c["ref_i8"], what + " int8 output")
            yf = _fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_F32, what)[0]
            np.testing.assert_allclose(yf, c["ref_f32"], rtol=1e-5, atol=0, err_msg=what + " fp32 output")
            mid, (tf, _) = _two_launches(gpu_ctx, capi, case, c, act, alpha)
            _eq(mid, c["mid"], what + " depthwise launch")
            _eq(yf, tf, what + " fp32 output against the two launches")
            ran += 1
    assert ran >= 2


@pytest.mark.parametrize("name", D.EDGE_CASES)
def test_graph_tail_on_its_value_edges(gpu_ctx, pkg, plref, name):
    """Calib copy alone, residual sum without and with relu; the fp32 sum kept, then dropped (y == NULL)."""
    capi, case = pkg.capi, D.BY_NAME[name]
    for j, (act, alpha, _seed) in enumerate(D.acts_of(case)):
        c = D.reference(plref, case, j)
        for key, t in c["tails"].items():
            what = "%s act %d tail %s" % (name, act, key)
            tail = dict(calib_scale=c["calib"])
            if t["res"] is not None:
                tail.update(residual=t["res"], residual_relu=int(t["relu"]))
            y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_F32, what, **tail)
            _eq(y, t["z"], what + " fp32 sum")
            _eq(yq, t["q"], what + " calib copy")
            _mid, (tf, tq) = _two_launches(gpu_ctx, capi, case, c, act, alpha, **tail)
            _eq(y, tf, what + " fp32 sum against the two launches")
            _eq(yq, tq, what + " calib copy against the two launches")
            y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_F32, what, want_y=False, **tail)
            assert y is None
            _eq(yq, t["q"], what + " calib copy, fp32 sum dropped")
        if j == 0:  # a residual without a calib copy
            t = c["tails"]["res_relu"]
            y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_F32, name, residual=t["res"], residual_relu=1)
            assert yq is None
            _eq(y, t["z"], name + " residual relu, no calib copy")


@pytest.mark.parametrize("name", D.EDGE_CASES)
def test_unaligned_outputs_keep_values_and_margins(gpu_ctx, pkg, plref, name):
    """y 1, 2, 3 elements and y_i8 1, 2, 3 bytes off their alignment, for every output kind (_fused checks the margins)."""
    capi, case = pkg.capi, D.BY_NAME[name]
    act, alpha, _seed = D.acts_of(case)[0]
    c = D.reference(plref, case, 0)
    t = c["tails"]["res"]
    for off in (1, 2, 3):
        what = "%s outputs off by %d" % (name, off)
        _eq(_fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_I32, what, y_off=off)[0], c["acc"], what + " int32")
        _eq(_fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_I8, what, y_off=off)[0], c["ref_i8"], what + " int8")
        y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_F32, what, y_off=off, q_off=off, residual=t["res"],
                       calib_scale=c["calib"])
        _eq(y, t["z"], what + " fp32 sum")
        _eq(yq, t["q"], what + " calib copy")
        y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_F32, what, q_off=4 - off, calib_scale=c["calib"], want_y=False)
        _eq(yq, c["tails"]["calib"]["q"], what + " calib copy alone")


@pytest.mark.parametrize("name", D.BATCH_CASES)
def test_batch_sweep_of_distinct_images(gpu_ctx, pkg, plref, name):
    """n in 1, 2, 3, 9 of nine distinct images, on a plan with several tiles per image and on one with a single tile: every
    image of every batch equals the oracle's image and its own batch-1 run, in the int8 output, the fp32 sum and the calib copy."""
    capi, case = pkg.capi, D.BY_NAME[name]
    act, alpha, seed = D.acts_of(case)[0]
    big = max(D.BATCH_NS)
    c = D.make(plref, case, act, alpha, seed, n=big)
    t = c["tails"]["res"]
    assert len({c["ref_i8"][b].tobytes() for b in range(big)}) == big

    def run(lo, hi):
        what = "%s images %d..%d" % (name, lo, hi - 1)
        y8 = _fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_I8, what, x=c["x"][lo:hi])[0]
        yf, yq = _fused(gpu_ctx, capi, case, c, act, alpha, capi.OUT_F32, what, x=c["x"][lo:hi], residual=t["res"][lo:hi],
                        calib_scale=c["calib"])
        return y8, yf, yq
    singles = [run(b, b + 1) for b in range(big)]
    for n in D.BATCH_NS:
        got = run(0, n)
        for b in range(n):
            for g, s, want, k in zip(got, singles[b], (c["ref_i8"], t["z"], t["q"]), ("int8 output", "fp32 sum", "calib copy")):
                _eq(g[b], want[b], "%s n=%d image %d %s" % (name, n, b, k))
                _eq(g[b], s[0], "%s n=%d image %d %s against its batch-1 run" % (name, n, b, k))
