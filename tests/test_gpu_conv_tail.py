"""GPU: the fused conv tail (plhip_conv2d_int8_fused) on every kernel and store path that takes it, on the cases of
tail_cases.py (test_tail_cases.py proves on the host that each case reaches the instance it names and that the operands reach
their edges).

Every case, every tail (calib copy alone, residual sum with and without relu, residual + relu without a calib copy), the fp32
sum kept and dropped: the fp32 sum and the calib copy equal the oracle's instruction sequence (conv2d_acc + epilogue,
elementwise_add, calib_f32_to_i8) bit for bit -- both sides do one fmaf on dyadic operands (test_gpu_edges.py) -- and are
byte-identical to the separate launches through the C ABI.  Non-dyadic operand sets hold the fp32 sum to rtol 1e-5 and the calib
copy to the oracle's calib of the fp32 values the launch returned.  The cases with stated seeds also run with each pointer alone
1, 2, 3 off its vector alignment, and three plans run a batch sweep of distinct images.  Every fused launch writes into
allocations filled with 0xA5 whose margins must come back untouched, so a value stored outside the tensor, or not stored at all,
cannot pass."""
import ctypes

import numpy as np
import pytest

import tail_cases as T

pytestmark = pytest.mark.gpu
POISON = 0xA5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq(got, want, what):
    assert got is not None and got.dtype == want.dtype and got.shape == want.shape, what
    bad = (_bits(got) != _bits(want)) if got.dtype == np.float32 else (got != want)
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %s want %s" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:6], want[bad][:6])


def _tail_args(c, key):
    """(residual, residual_relu, calib scale) of tail `key` of a made case."""
    use_res, relu, calib = T.TAILS[key]
    return (c["res"] if use_res else None), int(relu), (c["calib"] if calib else None)


def _fused(ctx, capi, case, c, act, alpha, key, what, want_f32=True, lo=None, hi=None, misalign=0):
    """One fused launch of tail `key` into poisoned, guarded outputs: (y, y_i8) after the margins of both were found untouched;
    lo, hi: the images of the made case that run."""
    sl = slice(lo, hi)
    x = c["x"][sl]
    d = T.desc_of(capi, case["shape"], act, alpha, n=x.shape[0])
    assert ctx.L.plhip_conv2d_fused_supported(ctypes.byref(d)) == 1, what
    assert ctx.L.plhip_conv_impl_name(ctypes.byref(d)).decode() == case["impl"], what
    res, relu, calib = _tail_args(c, key)
    y, yq, my, mq = ctx.conv2d_fused(d, x, c["w"], c["scale"], c["bias"], None if res is None else res[sl], relu, calib,
                                     want_f32=want_f32, misalign=misalign, sentinel=POISON)
    for m, name in ((my, "y"), (mq, "y_i8")):
        assert m is None or (m == POISON).all(), "%s: %d bytes written outside %s" % (what, (m != POISON).sum(), name)
    assert (y is None) == (not want_f32) and (yq is None) == (calib is None), what
    return y, yq


def _separate(ctx, capi, case, c, act, alpha, y0, key):
    """The launches the fused one replaces, on the fp32 conv output y0: elementwise_add (+ relu), calib."""
    res, relu, calib = _tail_args(c, key)
    z = y0 if res is None else ctx.elementwise_add(y0, res, bool(relu))
    return z, (None if calib is None else ctx.calib_f32_to_i8(z, calib))


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES])
def test_every_tail_equals_the_oracle_and_the_separate_launches(gpu_ctx, pkg, plref, name):
    capi, case = pkg.capi, T.BY_NAME[name]
    for j, (act, alpha, _seed) in enumerate(T.acts_of(case)):
        c = T.reference(plref, case, j)
        d = T.desc_of(capi, case["shape"], act, alpha)
        y0 = gpu_ctx.conv2d(d, c["x"], c["w"], c["scale"], c["bias"], capi.OUT_F32)
        _eq(y0, c["pre"], "%s act %d: plhip_conv2d_int8 fp32" % (name, act))
        for key, t in c["tails"].items():
            what = "%s act %d alpha %g tail %s" % (name, act, alpha, key)
            y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, key, what)
            sz, sq = _separate(gpu_ctx, capi, case, c, act, alpha, y0, key)
            _eq(y, t["z"], what + " fp32 sum")
            _eq(y, sz, what + " fp32 sum against the separate launches")
            if t["q"] is None:
                assert yq is None
                continue
            _eq(yq, t["q"], what + " calib copy")
            _eq(yq, sq, what + " calib copy against the separate launches")
            y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, key, what, want_f32=False)
            _eq(yq, t["q"], what + " calib copy, fp32 sum dropped")


@pytest.mark.parametrize("name,act,alpha", T.ND_CASES)
def test_nondyadic_scales_and_calib_scale(gpu_ctx, pkg, plref, name, act, alpha):
    """Scales and a calib scale (0.3) that are no powers of two: the fp32 sum within rtol 1e-5 of the oracle, the calib copy the
    oracle's calib of the fp32 values this launch returned -- the kernel multiplies by 1 / scale as the reference does -- and the
    copy of a launch that drops the fp32 sum (tr_stage_i8_calib on gemm_tr) that of the launch that kept it."""
    capi, case = pkg.capi, T.BY_NAME[name]
    c = T.reference_nondyadic(plref, name, act, alpha)
    for key, t in c["tails"].items():
        what = "%s act %d tail %s, non-dyadic" % (name, act, key)
        y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, key, what)
        np.testing.assert_allclose(y, t["z"], rtol=1e-5, atol=0, err_msg=what + " fp32 sum")
        if yq is None:
            continue
        _eq(yq, plref.calib_f32_to_i8(y, c["calib"]), what + " calib copy of the returned fp32 values")
        _y, yd = _fused(gpu_ctx, capi, case, c, act, alpha, key, what, want_f32=False)
        _eq(yd, yq, what + " calib copy, fp32 sum dropped")


@pytest.mark.parametrize("name", T.EDGE_CASES)
def test_each_pointer_off_its_alignment_keeps_values_and_margins(gpu_ctx, pkg, plref, name):
    """y, the residual, y_i8 (and x on the 1x1 cases) each alone 1, 2, 3 off their vector alignment, the others aligned: the
    scalar store forms under a tail (_fused checks the margins)."""
    capi, case = pkg.capi, T.BY_NAME[name]
    plan = T.plan_of(capi, case["shape"], T.TAIL_RES | T.TAIL_CALIB | T.TAIL_UNALIGNED)
    assert plan["kernel"] == case["kernel"] and plan.get("VS", 0) == 0
    refs = [T.reference(plref, case, j) for j in range(2)]
    acts = T.acts_of(case)
    slots = ("x", "y", "residual", "y_i8")
    for off in (1, 2, 3):
        for slot in range(0 if case["shape"][5] == 1 and case["impl"] == T.GEMM else 1, 4):
            # the residual sum under no activation (round_sat_i8); the relu'd sum under relu6 (the packed non-negative rounding)
            j, key = (0, "res") if slot != 3 else (1, "res_relu")
            (act, alpha, _seed), c = acts[j], refs[j]
            what = "%s %s off by %d, tail %s" % (name, slots[slot], off, key)
            mis = tuple(off if k == slot else 0 for k in range(4))
            y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, key, what, misalign=mis)
            _eq(y, c["tails"][key]["z"], what + " fp32 sum")
            _eq(yq, c["tails"][key]["q"], what + " calib copy")
        (act, alpha, _seed), c = acts[0], refs[0]
        what = "%s y_i8 off by %d, calib alone, fp32 dropped" % (name, off)
        _y, yq = _fused(gpu_ctx, capi, case, c, act, alpha, "calib", what, want_f32=False, misalign=(0, 0, 0, off))
        _eq(yq, c["tails"]["calib"]["q"], what)


@pytest.mark.parametrize("name", T.BATCH_CASES)
def test_batch_sweep_of_distinct_images(gpu_ctx, pkg, plref, name):
    """n in 1, 2, 3, 9 of nine distinct images: every image of every batch equals the oracle's image and its own batch-1 run, in
    the fp32 sum and in the calib copy."""
    capi, case = pkg.capi, T.BY_NAME[name]
    act, alpha, seed = T.acts_of(case)[0]
    big = max(T.BATCH_NS)
    c = T.make(plref, case, act, alpha, seed, n=big)
    t = c["tails"]["res"]
    assert len({t["q"][b].tobytes() for b in range(big)}) == big

    def run(lo, hi):
        return _fused(gpu_ctx, capi, case, c, act, alpha, "res", "%s images %d..%d" % (name, lo, hi - 1), lo=lo, hi=hi)
    singles = [run(b, b + 1) for b in range(big)]
    for n in T.BATCH_NS:
        got = run(0, n)
        for b in range(n):
            for g, s, want, k in zip(got, singles[b], (t["z"], t["q"]), ("fp32 sum", "calib copy")):
                _eq(g[b], want[b], "%s n=%d image %d %s" % (name, n, b, k))
                _eq(g[b], s[0], "%s n=%d image %d %s against its batch-1 run" % (name, n, b, k))


def test_refusals_launch_nothing(gpu_ctx, pkg, plref):
    """No output at all, a calib scale of 0 or below, residual_relu without a residual, a tail on the direct 3x3 stride-2 stem:
    the call returns its status and the poisoned outputs come back untouched."""
    capi = pkg.capi
    L = gpu_ctx.L

    def attempt(shape, what, want_status, y=True, q=True, res=True, relu=0, calib=0.5):
        d = T.desc_of(capi, shape)
        oh, ow = capi.out_hw(d)
        n, cin, h, w, cout, k = shape[:6]
        oshape = (n, cout, oh, ow)
        with gpu_ctx.scope() as s:
            dx = s.put(np.ones((n, cin, h, w), np.int8))
            ds, db = s.put(np.ones(cout, np.float32)), s.put(np.zeros(cout, np.float32))
            dr = s.put(np.ones(oshape, np.float32))
            yf, yq = s.out(oshape, np.float32, fill=POISON, guard=capi.MARGIN_GUARD), s.out(oshape, np.int8, fill=POISON, guard=capi.MARGIN_GUARD)
            dwp = gpu_ctx._packed_conv(s, d, np.ones((cout, cin // shape[9], k, k), np.int8))
            dws, wsb = gpu_ctx._conv_workspace(s, d)
            st = L.plhip_conv2d_int8_fused(gpu_ctx.h, ctypes.byref(d), dx, dwp, ds, db, yf.ptr if y else None, dr if res else None,
                                           relu, yq.ptr if q else None, float(calib), dws, wsb)
            gpu_ctx.sync()
            assert st == want_status, (what, st, L.plhip_last_error(gpu_ctx.h))
            for o in (yf, yq):
                assert (o.get().view(np.uint8) == POISON).all() and (o.margins() == POISON).all(), what
    INVALID, UNSUPPORTED = -1, -3  # PLHIP_ERR_INVALID, PLHIP_ERR_UNSUPPORTED (include/plhip.h)
    lds = T.BY_NAME["lds_6x6"]["shape"]
    attempt(lds, "no output at all", INVALID, y=False, q=False)
    attempt(lds, "calib scale 0", INVALID, calib=0.0)
    attempt(lds, "calib scale below 0", INVALID, calib=-0.5)
    attempt(lds, "calib scale NaN", INVALID, calib=float("nan"))
    attempt(lds, "residual_relu without a residual", INVALID, res=False, relu=1)
    attempt(T.BY_NAME["stat_a_7x7"]["shape"], "residual_relu without a residual, patch route", INVALID, res=False, relu=1)
    attempt(T.REFUSED_SHAPE, "a residual on the direct 3x3 stride-2 stem", UNSUPPORTED, q=False)
    attempt(T.REFUSED_SHAPE, "a calib copy on the direct 3x3 stride-2 stem", UNSUPPORTED, res=False)
