"""-m gpu: the MobileNetV3 ops on the device.  plhip_hard_act_f32 / plhip_se_scale_f32 against the numpy restatements of
mbv3_oracle.py bit for bit (fp32 and int8: every operation is an exactly rounded one), the kernel classes through
KernelFactory -> SetParam -> Launch, and MobileNetV3-Large / -Small whole programs against the helper oracle."""
import importlib

import numpy as np
import pytest

import glue_cases as G
import mbv3_oracle as M
from replay_cases import written

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_f32(got, want, what):
    """Bit-exact, NaN included (any NaN equals any NaN: the payload is not part of the contract)."""
    g, w = _bits(got), _bits(want)
    ok = (g == w) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), "%s: %d of %d fp32 values differ" % (what, (~ok).sum(), ok.size)


def _same_i8(gpu_ctx, got_q, want_f32, got_f32, scale, what):
    """The int8 output: the numpy restatement of calib wherever the fp32 value is a number, and everywhere (NaN included, whose
    int8 image the reference does not define) exactly what plhip_calib_f32_to_i8 makes of the fp32 output."""
    num = ~np.isnan(want_f32)
    want_q = M.calib_i8(want_f32, scale)
    assert np.array_equal(got_q[num], want_q[num]), "%s: %d int8 values differ" % (what, (got_q[num] != want_q[num]).sum())
    assert np.array_equal(got_q, gpu_ctx.calib_f32_to_i8(got_f32, scale)), what + ": differs from the separate calib call"


def _inputs(rng, count):
    x = (rng.standard_normal(count) * 4).astype(F32)
    edge = np.array([-3, 3, 0, -0.0, -2.5, 2.5, np.nextafter(F32(-3), F32(0)), np.nextafter(F32(-3), F32(-4)), np.nextafter(F32(3), F32(4)),
                     np.nextafter(F32(3), F32(0)), np.nan, np.inf, -np.inf, 1e-40, -1e-40, 3e38, -3e38, 1e-20], F32)
    k = min(count, edge.size)
    x[:k] = edge[:k]
    return x


@pytest.mark.parametrize("kind", ["hard_swish", "hard_sigmoid"])
def test_hard_act_bit_exact(gpu_ctx, pkg, kind):
    capi = pkg.capi
    rng = np.random.default_rng(360)
    k = capi.HARD_SWISH if kind == "hard_swish" else capi.HARD_SIGMOID
    ref_fn = M.hard_swish if kind == "hard_swish" else M.hard_sigmoid
    scale = 12.0 / 127 if kind == "hard_swish" else 1.0 / 127
    for count in (1, 3, 4, 5, 49, 1023, 4096, 16 * 56 * 56 + 2, 2 * 240 * 28 * 28):
        x = _inputs(rng, count)
        want = ref_fn(x)
        for mis in (0, 1):  # aligned bases: the vector path; bases off by one element: the scalar loop
            yf, _ = gpu_ctx.hard_act(k, x, mode="f32", misalign=mis)
            _, yq = gpu_ctx.hard_act(k, x, mode="i8", calib_scale=scale, misalign=mis)
            bf, bq = gpu_ctx.hard_act(k, x, mode="both", calib_scale=scale, misalign=mis)
            _same_f32(yf, want, "%s count %d misalign %d" % (kind, count, mis))
            _same_i8(gpu_ctx, yq, want, yf, scale, "%s count %d misalign %d" % (kind, count, mis))
            _same_f32(bf, yf, "both-outputs fp32")
            assert np.array_equal(bq, yq)
    # other parameters than the defaults
    x = _inputs(rng, 5000)
    if kind == "hard_swish":
        yf, _ = gpu_ctx.hard_act(k, x, params=(4.0, 5.0, 2.0))
        _same_f32(yf, M.hard_swish(x, 4.0, 5.0, 2.0), "hard_swish params")
    else:
        yf, _ = gpu_ctx.hard_act(k, x, params=(0.1666667, 0.5))
        _same_f32(yf, M.hard_sigmoid(x, 0.1666667, 0.5), "hard_sigmoid params")


def test_hard_act_refuses_bad_arguments(gpu_ctx, pkg):
    import ctypes as C
    capi = pkg.capi
    L = capi.load()
    pr = (C.c_float * 3)(6, 6, 3)
    with gpu_ctx.scope() as s:
        d = s.alloc(64)
        assert L.plhip_hard_act_f32(gpu_ctx.h, 0, pr, d, None, None, 1.0, 4) < 0       # no output
        assert L.plhip_hard_act_f32(gpu_ctx.h, 0, pr, d, None, d, 0.0, 4) < 0          # int8 output without a scale
        assert L.plhip_hard_act_f32(gpu_ctx.h, 7, pr, d, d, None, 1.0, 4) < 0          # unknown kind
        assert L.plhip_se_scale_f32(gpu_ctx.h, d, d, 1, 0, 4, d, None, 1.0) < 0
        assert L.plhip_se_scale_f32(gpu_ctx.h, d, None, 1, 1, 4, d, None, 1.0) < 0


@pytest.mark.parametrize("hw", [1, 9, 16, 25, 49, 64, 196, 3136])  # 1, 16, 64 and 256 lanes per plane, scalar and vector
def test_se_scale_bit_exact(gpu_ctx, hw):
    rng = np.random.default_rng(361 + hw)
    for (n, c) in ((1, 16), (3, 72), (2, 184), (2, 960)):
        x = _inputs(rng, n * c * hw).reshape(n, c, hw)
        g = rng.uniform(0, 1, (n, c)).astype(F32)
        g.flat[:3] = [0, 1, 0.5]
        want = M.se_scale(x, g)
        scale = 8.0 / 127
        for mis in (0, 1):
            yf, _ = gpu_ctx.se_scale(x, g, mode="f32", misalign=mis)
            _, yq = gpu_ctx.se_scale(x, g, mode="i8", calib_scale=scale, misalign=mis)
            bf, bq = gpu_ctx.se_scale(x, g, mode="both", calib_scale=scale, misalign=mis)
            _same_f32(yf, want, "se_scale n %d c %d hw %d misalign %d" % (n, c, hw, mis))
            _same_i8(gpu_ctx, yq, want, yf, scale, "se_scale n %d c %d hw %d misalign %d" % (n, c, hw, mis))
            _same_f32(bf, yf, "both-outputs fp32")
            assert np.array_equal(bq, yq)


def _se_pairs(wl):
    """Every (C, Cr) of the squeeze-excite blocks of both networks."""
    pairs = set()
    for table in (wl.MBV3_LARGE, wl.MBV3_SMALL):
        pairs |= {(exp, wl.mbv3_squeeze_channels(exp)) for (_k, exp, _c, se, _hs, _s) in table if se}
    return sorted(pairs)


@pytest.mark.parametrize("batch", [1, 3, 128])
def test_se_gate_equals_the_separate_calls(gpu_ctx, pkg, wl, batch):
    """plhip_se_gate_int8 against calib -> conv 1x1 [int8] -> conv 1x1 [fp32] -> hard_sigmoid through the separate C ABI calls,
    byte for byte, over every (C, Cr) pair of both networks; the gate must use both clamps and the ramp.  Then over pairs outside
    the tables (glue_cases.SE_EXTRA_PAIRS): the kernel promises any C, Cr in 8..960."""
    capi = pkg.capi
    pairs = _se_pairs(wl)
    assert (72, 24) in pairs and (960, 240) in pairs and (16, 8) in pairs and len(pairs) >= 11
    rng = np.random.default_rng(370 + batch)
    for (c, cr) in pairs:
        pooled = rng.uniform(-0.5, 3.0, (batch, c)).astype(F32)
        scale = F32(3.0 / 127)
        w1 = rng.integers(-127, 128, (cr, c, 1, 1)).astype(np.int8)
        w2 = rng.integers(-127, 128, (c, cr, 1, 1)).astype(np.int8)
        var1, var2 = (1 + np.arange(cr) % 7 / 8.0), (1 + np.arange(c) % 7 / 8.0)
        s1 = (var1 * 40.0 / (np.sqrt(c) * 60 * 73)).astype(F32)
        b1 = rng.uniform(-20, 20, cr).astype(F32)
        s2 = (var2 * 2.8 / (np.sqrt(cr) * 30 * 73)).astype(F32)
        b2 = rng.uniform(-1, 1, c).astype(F32)
        for act1, alpha1 in ((capi.ACT_RELU, 0.0), (capi.ACT_RELU6, 90.0)):
            q = gpu_ctx.calib_f32_to_i8(pooled.reshape(batch, c, 1, 1), float(scale))
            d1 = capi.conv_desc(batch, c, 1, 1, cr, 1, 1, act=act1, alpha=alpha1)
            mid = gpu_ctx.conv2d(d1, q, w1, s1, b1, capi.OUT_I8)
            d2 = capi.conv_desc(batch, cr, 1, 1, c, 1, 1)
            y = gpu_ctx.conv2d(d2, mid, w2, s2, b2, capi.OUT_F32)
            want, _ = gpu_ctx.hard_act(capi.HARD_SIGMOID, y.reshape(batch, c))
            got = gpu_ctx.se_gate(pooled, float(scale), w1, s1, b1, act1, alpha1, w2, s2, b2)
            assert np.array_equal(_bits(got), _bits(want)), "c %d cr %d batch %d act %d: %d gates differ" % (
                c, cr, batch, act1, (_bits(got) != _bits(want)).sum())
            _same_f32(want, M.hard_sigmoid(y.reshape(batch, c)), "hard_sigmoid of the separate calls")
            if batch * c >= 48:
                assert (got == 0).any() and (got == 1).any() and ((got > 0) & (got < 1)).any(), (c, cr)
    # no bias: the convs take NULL too
    c, cr = 72, 24
    pooled = rng.uniform(0, 3, (batch, c)).astype(F32)
    w1 = rng.integers(-127, 128, (cr, c, 1, 1)).astype(np.int8)
    w2 = rng.integers(-127, 128, (c, cr, 1, 1)).astype(np.int8)
    s1, s2 = np.full(cr, 1e-4, F32), np.full(c, 2e-4, F32)
    q = gpu_ctx.calib_f32_to_i8(pooled.reshape(batch, c, 1, 1), 0.025)
    mid = gpu_ctx.conv2d(capi.conv_desc(batch, c, 1, 1, cr, 1, 1, act=capi.ACT_RELU), q, w1, s1, None, capi.OUT_I8)
    y = gpu_ctx.conv2d(capi.conv_desc(batch, cr, 1, 1, c, 1, 1), mid, w2, s2, None, capi.OUT_F32)
    want, _ = gpu_ctx.hard_act(capi.HARD_SIGMOID, y.reshape(batch, c))
    assert np.array_equal(_bits(gpu_ctx.se_gate(pooled, 0.025, w1, s1, None, capi.ACT_RELU, 0.0, w2, s2, None)), _bits(want))
    # outside the network tables: C and Cr that are no multiples of 4 (both int8 vectors are zero padded in k), the ends of
    # the 8..960 envelope.  Nonzero weights in the last input channel of each conv: a padding byte that is not zero moves a gate.
    rng = np.random.default_rng(380 + batch)
    for (c, cr) in G.SE_EXTRA_PAIRS:
        assert (c, cr) not in pairs
        pooled = rng.uniform(-0.5, 3.0, (batch, c)).astype(F32)
        scale = F32(3.0 / 127)
        w1 = rng.integers(-127, 128, (cr, c, 1, 1)).astype(np.int8)
        w2 = rng.integers(-127, 128, (c, cr, 1, 1)).astype(np.int8)
        w1[:, -1][w1[:, -1] == 0] = 77
        w2[:, -1][w2[:, -1] == 0] = -77
        var1, var2 = (1 + np.arange(cr) % 7 / 8.0), (1 + np.arange(c) % 7 / 8.0)
        s1 = (var1 * 40.0 / (np.sqrt(c) * 60 * 73)).astype(F32)
        b1 = rng.uniform(-20, 20, cr).astype(F32)
        s2 = (var2 * 2.8 / (np.sqrt(cr) * 30 * 73)).astype(F32)
        b2 = rng.uniform(-1, 1, c).astype(F32)
        for act1, alpha1 in ((capi.ACT_RELU, 0.0), (capi.ACT_RELU6, 90.0)):
            assert gpu_ctx.L.plhip_se_gate_supported(c, cr, act1, capi.ACT_NONE) == 1, (c, cr)
            q = gpu_ctx.calib_f32_to_i8(pooled.reshape(batch, c, 1, 1), float(scale))
            mid = gpu_ctx.conv2d(capi.conv_desc(batch, c, 1, 1, cr, 1, 1, act=act1, alpha=alpha1), q, w1, s1, b1, capi.OUT_I8)
            y = gpu_ctx.conv2d(capi.conv_desc(batch, cr, 1, 1, c, 1, 1), mid, w2, s2, b2, capi.OUT_F32)
            want, _ = gpu_ctx.hard_act(capi.HARD_SIGMOID, y.reshape(batch, c))
            got = gpu_ctx.se_gate(pooled, float(scale), w1, s1, b1, act1, alpha1, w2, s2, b2)
            assert np.array_equal(_bits(got), _bits(want)), "c %d cr %d batch %d act %d: %d gates differ" % (
                c, cr, batch, act1, (_bits(got) != _bits(want)).sum())
            _same_f32(want, M.hard_sigmoid(y.reshape(batch, c)), "hard_sigmoid of the separate calls")
            if batch * c >= 48:
                assert ((got > 0) & (got < 1)).any(), (c, cr)  # gates on the ramp: every accumulator bit shows


def test_kernel_classes_through_the_factory(lite):
    """KernelFactory -> SetParam -> Launch for the three ops, the def alias and the int8 alias (calib tail), and the kernel
    names they report; then the refusal of a broadcast the multiply does not have."""
    rng = np.random.default_rng(362)
    x = (rng.standard_normal((2, 72, 14, 14)) * 4).astype(F32)
    p = lite.Predictor(0)
    try:
        p.add_feed("x", x.shape)
        p.add_io_copy("x", "xd", True)
        p.add_global_avg_pool("xd", "pool")
        p.add_activation("hard_swish", "xd", "hs")
        p.add_activation("hard_swish", "xd", "hs2", calib_out="hs2_q", calib_scale=0.1)
        p.add_activation("hard_swish", "xd", "hs3", calib_out="hs3_q", calib_scale=0.1, drop_fp32=True)
        p.add_activation("hard_sigmoid", "pool", "gate")
        p.add_elementwise_mul("hs", "gate", "prod", 0)
        p.add_elementwise_mul("hs", "gate", "prod2", 0, calib_out="prod2_q", calib_scale=0.05, drop_fp32=True)
        p.add_elementwise_mul("hs", "hs", "sq", -1)
        p.set_input("x", x)
        p.run()
        p.run()
        names = "\n".join(p.kernel_names())
        for frag in ("/def -> hard_swish_hip", "/int8 -> hard_swish_fp32_int8_hip", "/int8 -> hard_swish_int8_hip",
                     "/def -> hard_sigmoid_hip", "/def -> se_scale_hip", "/int8 -> se_scale_int8_hip"):
            assert frag in names, (frag, names)
        hs = M.hard_swish(x)
        _same_f32(p.get_var("hs", F32), hs, "hard_swish class")
        _same_f32(p.get_var("hs2", F32), hs, "hard_swish int8 alias, fp32 output")
        assert np.array_equal(p.get_var("hs2_q", np.int8), M.calib_i8(hs, 0.1))
        assert np.array_equal(p.get_var("hs3_q", np.int8), M.calib_i8(hs, 0.1))
        pool = p.get_var("pool", F32)
        gate = M.hard_sigmoid(pool)
        _same_f32(p.get_var("gate", F32), gate, "hard_sigmoid class")
        prod = M.se_scale(hs, gate)
        _same_f32(p.get_var("prod", F32), prod, "elementwise_mul class")
        assert np.array_equal(p.get_var("prod2_q", np.int8), M.calib_i8(prod, 0.05))
        _same_f32(p.get_var("sq", F32), (hs * hs).astype(F32), "elementwise_mul, equal shapes")
    finally:
        p.close()
    q = lite.Predictor(0)
    try:
        q.add_feed("x", (2, 8, 4, 4))
        q.add_feed("y", (2, 1, 4, 4))
        q.add_io_copy("x", "xd", True)
        q.add_io_copy("y", "yd", True)
        q.add_elementwise_mul("xd", "yd", "o", 0)
        q.set_input("x", np.zeros((2, 8, 4, 4), F32))
        q.set_input("y", np.zeros((2, 1, 4, 4), F32))
        with pytest.raises(lite.LiteError, match="unsupported broadcast"):
            q.run()
    finally:
        q.close()


def _run(lite, wl, net, img, fuse, fuse_hard_act=None):
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, img.shape[0], fuse=fuse, fuse_hard_act=fuse_hard_act)
        plan = p.graph_plan()
        assert p.graph_lower() == [out]
        p.set_input(net["input"], img)
        p.run()
        p.run()
        return p, out, plan
    except Exception:
        p.close()
        raise


def _check(p, name, want, out):
    got = p.get_var(name, want.dtype)
    assert got.shape == want.shape, name
    if want.dtype == np.int8:
        assert np.array_equal(got, want), "%s: %d of %d int8 values differ" % (name, (got != want).sum(), want.size)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-4 if name == out else 1e-5, atol=1e-5, err_msg=name)


@pytest.mark.parametrize("variant,n_se", [("large", 8), ("small", 9)])
def test_mobilenet_v3_program_vs_oracle(lite, wl, plref, variant, n_se):
    """Batch 2, variable by variable: every int8 tensor bit for bit, every fp32 tensor within 1e-5; unfused (the reference's
    instruction list), fused by default, and fused with J1 / J2 / J3.  Every variable a fused plan says it writes is required and
    equals the unfused program's byte for byte."""
    net = wl.mobilenet_v3_net(variant)
    img = np.random.default_rng(350).uniform(-1, 1, (2, 3, 224, 224)).astype(F32)
    ref = M.forward(plref, net, img)
    ref = {k: v.reshape(v.shape[0], -1, 1, 1) if k.endswith("_se_pool") or k == "pool" else v for k, v in ref.items()}
    pu, out, plan_u = _run(lite, wl, net, img, fuse=False)
    try:
        names = "\n".join(pu.kernel_names())
        assert "hard_swish_hip" in names and "hard_sigmoid_hip" in names and "se_scale_hip" in names
        assert {n for n in written(plan_u) if "/target_trans" not in n} == set(ref)
        for name, want in ref.items():
            _check(pu, name, want, "prob")
        for fha in (None, True):
            pf, outf, plan_f = _run(lite, wl, net, img, fuse=True, fuse_hard_act=fha)
            try:
                fnames = "\n".join(pf.kernel_names())
                if fha:
                    assert fnames.count("se_gate_int8_dot4_hip") == n_se and fnames.count("se_scale_int8_hip") == n_se
                    assert "hard_swish_int8_hip" in fnames and (variant != "large" or "hard_swish_fp32_int8_hip" in fnames)
                else:
                    assert not [k for k in ("se_gate_int8_dot4_hip", "hard_swish_int8_hip", "hard_swish_fp32_int8_hip", "se_scale_int8_hip") if k in fnames]
                survive = sorted(n for n in written(plan_f) if n in ref)
                gone = set(ref) - set(survive)
                assert len(survive) > len(ref) // 2
                if fha:  # J2 drops three tensors per block, J3's product is not written; J1's int8 outputs must be there
                    assert {n for n in gone if "_se_" in n} == {b + s for b in {g[:-len("_se_gate")] for g in ref if g.endswith("_se_gate")}
                                                                for s in ("_se_pool/precision_trans", "_se_reduce", "_se_expand", "_se_mul")}
                    assert all(n in survive for n in ref if n.endswith(("_hs/precision_trans", "_se_mul/precision_trans", "_se_gate")))
                for name in survive:
                    want = ref[name]
                    got = pf.get_var(name, want.dtype)
                    assert got.shape == want.shape, name
                    assert np.array_equal(got.view(np.uint8), pu.get_var(name, want.dtype).view(np.uint8)), name
            finally:
                pf.close()
    finally:
        pu.close()


def test_mobilenet_v3_large_at_batch_128(lite, wl, plref):
    """The program fused with J1 / J2 / J3 at the benchmark batch: the first two images reproduce the batch-2 run, image 77 equals
    the oracle; over every variable the plan says it writes."""
    B, mid = 128, 77
    net = wl.mobilenet_v3_net("large")
    img = np.random.default_rng(351).uniform(-1, 1, (B, 3, 224, 224)).astype(F32)
    ref_mid = M.forward(plref, net, img[mid:mid + 1], via_gemm=True)
    small, out, plan_s = _run(lite, wl, net, img[:2], fuse=True, fuse_hard_act=True)
    try:
        big, out_b, plan_b = _run(lite, wl, net, img, fuse=True, fuse_hard_act=True)
        try:
            assert [l.split(" ")[0] for l in plan_b] == [l.split(" ")[0] for l in plan_s]
            names = sorted(n for n in written(plan_b) if n in ref_mid)
            assert len(names) > 60, len(names)
            for name in names:
                want = ref_mid[name]
                s_ = small.get_var(name, want.dtype)
                g_ = big.get_var(name, want.dtype, max_bytes=int(want.nbytes) * B + 64)
                assert g_.shape[0] == B and s_.shape[0] == 2, name
                assert np.array_equal(g_[:2].view(np.uint8), s_.view(np.uint8)), "%s: batch-%d prefix differs from the batch-2 run" % (name, B)
                want = want.reshape(g_[mid:mid + 1].shape)
                if want.dtype == np.int8:
                    assert np.array_equal(g_[mid:mid + 1], want), "%s: image %d differs from the oracle" % (name, mid)
                else:
                    np.testing.assert_allclose(g_[mid:mid + 1], want, rtol=1e-4 if name == "prob" else 1e-5, atol=1e-5, err_msg=name)
        finally:
            big.close()
    finally:
        small.close()
