"""-m gpu: concat -> calib in one launch (plhip_concat_calib_f32) on the device, and fusion L around it.  The C ABI call against
shuffle_oracle.concat + calib_i8 (fp32 compared as uint32, int8 exactly) and against the two calls it replaces on the device (NaN
and infinities included), on every item width the host picks (16 floats, quads, elements), with more than 8 operands, one row
over many blocks, the axis-0 form and every base off alignment by one element; the refusals; the kernel class through
KernelFactory -> SetParam -> Launch; SqueezeNet v1.1 and the inception net as whole programs against the helper oracle, with L
against the unfused program and against L off."""
import ctypes as C
import importlib

import numpy as np
import pytest

import shuffle_oracle as S

pytestmark = pytest.mark.gpu
F32 = np.float32
SCALES = (4.0 / 127, 0.03125)  # the networks' scale, and a power of two: (k + 0.5) * scale times 1 / scale is a tie exactly


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _inputs(rng, shape, scale, nonfinite=False):
    """randn * 2 (a real share beyond +-127 steps of either scale) with the ties (k + 0.5) * scale, k = 0 .. 127, in both signs
    (+-127.5 * scale among them), values far outside the range, denormals and +-0 planted; nonfinite: NaN (two payloads) and +-inf too."""
    x = (rng.standard_normal(shape) * 2).astype(F32)
    flat = x.reshape(-1)
    k = np.arange(0, 128, dtype=np.float64)
    ties = np.concatenate([(k + 0.5) * scale, -(k + 0.5) * scale]).astype(F32)   # +-0.5 .. +-127.5 steps
    edge = np.concatenate([np.array([0.0, -0.0, 127.5 * scale, -127.5 * scale, 1e30, -1e30, 3e38, -3e38, 1000.0, -1000.0, 1e-40, -1e-40], F32), ties])
    if nonfinite:
        edge = np.concatenate([np.array([np.nan, np.inf, -np.inf, np.nan], F32), edge])
    n = min(flat.size, edge.size)
    pos = rng.permutation(flat.size)[:n]
    flat[pos] = edge[:n]
    if nonfinite:
        flat.view(np.uint32)[pos[0]] = 0x7FC12345  # a NaN with a payload of its own
    return x


def _many(count):
    return tuple(1 + (i * 5) % 6 for i in range(count))  # extents 1..6


# (outer, extents, inner): None as outer = the axis-0 form
CASES = [(1, (1,), 1),
         (2, (4, 8), 49),            # quads, rows no multiple of 16
         (2, (16, 16), 169),         # 16 floats per lane on a 13 x 13 plane
         (3, (3, 5), 7),             # elements
         (2, (4, 3), 49), (2, (3, 4), 49),   # one operand's rows no multiple of 4, behind and in front of one that is
         (2, _many(8), 16), (2, _many(9), 16), (2, _many(17), 16),   # one launch, two and three launches inside the call
         (1, (64, 64), 3025),        # one row over many blocks (fire2 / fire3 of SqueezeNet, one image)
         (None, (2, 3), 245)]


def _operands(rng, outer, extents, inner, scale, nonfinite=False):
    if outer is None:
        return [_inputs(rng, (c, inner), scale, nonfinite) for c in extents], 0
    return [_inputs(rng, (outer, c, inner), scale, nonfinite) for c in extents], 1


@pytest.mark.parametrize("outer,extents,inner", CASES)
def test_concat_calib_equals_the_oracle_and_the_two_calls(gpu_ctx, outer, extents, inner):
    rng = np.random.default_rng(560 + sum(extents) + inner + len(extents))
    for scale in SCALES:
        xs, axis = _operands(rng, outer, extents, inner, scale)
        want_f = S.concat(xs, axis)
        want_q = S.calib_i8(want_f, scale)
        if want_f.size >= 16:
            assert want_q.min() == -127 and want_q.max() == 127   # the planted values saturate on both sides
        ys, axis = _operands(rng, outer, extents, inner, scale, nonfinite=True)
        ab_f = gpu_ctx.concat(ys, axis)                       # the two calls the one launch replaces, on the device
        ab_q = gpu_ctx.calib_f32_to_i8(ab_f, scale)
        for mis in (0, 1):
            for with_f32 in (True, False):
                what = "concat_calib %s scale %g misalign %d f32 %d" % ((outer, extents, inner), scale, mis, with_f32)
                yf, yq = gpu_ctx.concat_calib(xs, axis, scale, with_f32=with_f32, misalign=mis)
                assert yq.shape == want_q.shape and yq.dtype == np.int8, what
                assert np.array_equal(yq, want_q), "%s: %d of %d int8 values differ from the oracle" % (what, (yq != want_q).sum(), want_q.size)
                assert not (yq == -128).any(), what
                if with_f32:
                    assert np.array_equal(_bits(yf), _bits(want_f)), what + ": fp32 bits moved wrongly"
                else:
                    assert yf is None
                zf, zq = gpu_ctx.concat_calib(ys, axis, scale, with_f32=with_f32, misalign=mis)
                assert zq.tobytes() == ab_q.tobytes(), "%s: %d int8 values differ from concat + calib on the device" % (what, (zq != ab_q).sum())
                assert not (zq == -128).any(), what
                if with_f32:
                    assert zf.tobytes() == ab_f.tobytes(), what + ": fp32 differs from plhip_concat_f32"


def test_bad_arguments_are_refused_before_any_launch(gpu_ctx, pkg):
    L = pkg.capi.load()
    h = gpu_ctx.h
    with gpu_ctx.scope() as s:
        src = s.put(np.arange(1024, dtype=F32))
        out_f, out_q = s.alloc(4096), s.alloc(4096)
        gpu_ctx.check(L.plhip_memset(h, out_f, 0x55, 4096), "memset")
        gpu_ctx.check(L.plhip_memset(h, out_q, 0x55, 4096), "memset")
        null = C.c_void_p()
        two = (C.c_void_p * 2)(src, src)
        one_null = (C.c_void_p * 2)(src, null)

        def ext(*v):
            return (C.c_int64 * len(v))(*v)

        def refused(words, *args):
            st = L.plhip_concat_calib_f32(h, *args)
            msg = L.plhip_last_error(h).decode()
            assert st < 0 and msg.startswith("plhip_concat_calib_f32: ") and words in msg, (st, msg, words)

        refused("count", two, ext(2, 3), 0, 1, 4, out_f, out_q, 1.0)
        refused("count", two, ext(2, 3), -1, 1, 4, out_f, out_q, 1.0)
        refused("null input", one_null, ext(2, 3), 2, 1, 4, out_f, out_q, 1.0)
        refused("extent", two, ext(2, 0), 2, 1, 4, out_f, out_q, 1.0)
        refused("extent", two, ext(-1, 3), 2, 1, 4, out_f, out_q, 1.0)
        refused("outer and inner", two, ext(2, 3), 2, 0, 4, out_f, out_q, 1.0)
        refused("outer and inner", two, ext(2, 3), 2, 1, 0, out_f, out_q, 1.0)
        refused("y_i8", two, ext(2, 3), 2, 1, 4, out_f, null, 1.0)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused("calib_scale", two, ext(2, 3), 2, 1, 4, out_f, out_q, bad)
        refused("2^40", two, ext(1 << 30, 1 << 30), 2, 1 << 30, 4, out_f, out_q, 1.0)
        refused("null", None, ext(2, 3), 2, 1, 4, out_f, out_q, 1.0)
        gpu_ctx.sync()
        # nothing was launched: both outputs still hold the fill
        assert (gpu_ctx.to_host(out_f, (4096,), np.uint8) == 0x55).all() and (gpu_ctx.to_host(out_q, (4096,), np.uint8) == 0x55).all()
        # and the same call with good arguments, with and without the fp32 output, is taken
        assert L.plhip_concat_calib_f32(h, two, ext(2, 3), 2, 1, 4, out_f, out_q, 1.0) == 0
        assert L.plhip_concat_calib_f32(h, two, ext(2, 3), 2, 1, 4, null, out_q, 1.0) == 0
        gpu_ctx.sync()
        want = np.concatenate([np.arange(8), np.arange(12)]).astype(np.int8)
        assert np.array_equal(gpu_ctx.to_host(out_q, (20,), np.int8), want)
        assert np.array_equal(gpu_ctx.to_host(out_f, (20,), F32), want.astype(F32))


def test_kernel_class_through_the_factory(lite):
    rng = np.random.default_rng(561)
    scale = SCALES[0]
    a, b, c = (_inputs(rng, (2, ch, 5, 7), scale, nonfinite=True) for ch in (6, 2, 4))
    p = lite.Predictor(0)
    try:
        for name, v in (("a", a), ("b", b), ("c", c)):
            p.add_feed(name, v.shape)
            p.add_io_copy(name, name + "d", True)
        p.add_concat_calib(["ad", "bd", "cd"], "cat", 1, "cat_q", scale, False)
        p.add_concat_calib(["ad", "bd", "cd"], "cat_dropped", 1, "cat_dq", scale, True)
        p.add_concat_calib(["ad", "ad"], "cat0", 0, "cat0_q", scale, False)
        p.add_concat(["ad", "bd", "cd"], "sep", 1)
        p.add_calib("sep", "sep_q", scale, True)
        for name, v in (("a", a), ("b", b), ("c", c)):
            p.set_input(name, v)
        p.run()
        p.run()
        names = "\n".join(p.kernel_names())
        assert names.count("/int8 -> concat_fp32_int8_hip") == 2 and names.count("/int8 -> concat_int8_hip") == 1, names
        want = S.concat([a, b, c], 1)
        assert np.array_equal(_bits(p.get_var("cat", F32)), _bits(want))
        q = p.get_var("cat_q", np.int8)
        num = ~np.isnan(want)
        assert q.shape == want.shape and np.array_equal(q[num], S.calib_i8(want, scale)[num])
        assert q.tobytes() == p.get_var("sep_q", np.int8).tobytes()
        assert p.get_var("cat_dq", np.int8).tobytes() == q.tobytes()
        want0 = S.concat([a, a], 0)
        assert np.array_equal(_bits(p.get_var("cat0", F32)), _bits(want0))
        assert np.array_equal(p.get_var("cat0_q", np.int8)[~np.isnan(want0)], S.calib_i8(want0, scale)[~np.isnan(want0)])
    finally:
        p.close()


# ------------------------------------------------------------------ whole programs
def _run(lite, wl, net, img, **kw):
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, img.shape[0], **kw)
        plan = p.graph_plan()
        assert p.graph_lower() == [out]
        assert p.num_instructions() == len(plan)
        p.set_input(net["input"], img)
        p.run()
        p.run()
        return p, out, plan
    except Exception:
        p.close()
        raise


def _written(plan):
    """The device variables a plan writes, read off its lines: every out= (not behind -f32, not the host copy) and +calib=."""
    names = set()
    for l in plan:
        toks = l.split(" ")
        kv = dict(f.split("=", 1) for f in toks[1:] if "=" in f)
        if l.startswith("io_copy/device_to_host"):
            continue
        if "-f32" not in toks:
            names.update(kv["out"].split(","))
        if "+calib" in kv:
            names.add(kv["+calib"])
    return names


def _ref(plref, net, img, gap):
    return {k: v.reshape(v.shape[0], -1, 1, 1) if k == gap else v for k, v in S.forward(plref, net, img).items()}


def _check(p, name, want):
    got = p.get_var(name, want.dtype)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if want.dtype == np.int8:
        assert np.array_equal(got, want), "%s: %d of %d int8 values differ" % (name, (got != want).sum(), want.size)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5, err_msg=name)


def _program_case(lite, wl, net, img, ref, n_int8, n_pool_int8, n_def):
    """Unfused against the oracle; default fused (L on) against the oracle, and byte for byte against the unfused program and
    against L off on every variable that survives."""
    pu, out, plan_u = _run(lite, wl, net, img, fuse=False)
    try:
        assert {n for n in _written(plan_u) if "/target_trans" not in n} == set(ref)
        for name, want in ref.items():
            _check(pu, name, want)
        po, _, plan_o = _run(lite, wl, net, img, fuse=True, fuse_concat=False)
        try:
            assert not [l for l in plan_o if l.startswith("concat/int8")]
            pf, _, plan_f = _run(lite, wl, net, img, fuse=True)  # the builder's defaults: L on
            try:
                pp = lite.Predictor(planner=True)
                try:
                    wl.emit_graph(pp, net, img.shape[0], fuse=True, fuse_concat=True)
                    assert pp.graph_plan() == plan_f
                finally:
                    pp.close()
                heads = [l.split(" ")[0] for l in plan_f]
                assert heads.count("concat/int8") == n_int8 and heads.count("concat/def") == n_def
                assert len([l for l in plan_f if l.startswith("pool2d/") and l.endswith(" int8")]) - \
                    len([l for l in plan_o if l.startswith("pool2d/") and l.endswith(" int8")]) == n_pool_int8
                assert "\n".join(pf.kernel_names()).count("/int8 -> concat_int8_hip") == n_int8
                survive = sorted(n for n in _written(plan_f) if n in ref)
                assert all(n in survive for n, v in ref.items() if v.dtype == np.int8 and not n.startswith(net["input"]))
                assert out[:-len("/host")] in survive and len(survive) > len(ref) // 2
                for name in survive:
                    _check(pf, name, ref[name])
                    got = pf.get_var(name, ref[name].dtype).tobytes()
                    assert got == pu.get_var(name, ref[name].dtype).tobytes(), name + ": L differs from the unfused program"
                    if name in _written(plan_o):
                        assert got == po.get_var(name, ref[name].dtype).tobytes(), name + ": L on differs from L off"
            finally:
                pf.close()
        finally:
            po.close()
    finally:
        pu.close()


@pytest.fixture(scope="module")
def squeezenet(wl):
    return wl.squeezenet_v1_1_net()


@pytest.fixture(scope="module")
def img224():
    return np.random.default_rng(350).uniform(-1, 1, (2, 3, 224, 224)).astype(F32)


@pytest.fixture(scope="module")
def ref224(plref, squeezenet, img224):
    return _ref(plref, squeezenet, img224, "pool10")


def test_squeezenet_v1_1_program_vs_oracle(lite, wl, squeezenet, img224, ref224):
    """224 x 224, batch 2: every concat becomes concat/int8 without its fp32 tensor, the pools behind fire3 and fire5 run on int8."""
    _program_case(lite, wl, squeezenet, img224, ref224, n_int8=8, n_pool_int8=2, n_def=0)


def test_inception_mini_program_vs_oracle(lite, wl, plref):
    """64 x 64, batch 2: the four-operand concat with a calib and a max pool behind it; the last concat stays concat/def."""
    net = wl.inception_mini_net()
    img = np.random.default_rng(350).uniform(-1, 1, (2, 3, 64, 64)).astype(F32)
    _program_case(lite, wl, net, img, _ref(plref, net, img, "pool"), n_int8=1, n_pool_int8=1, n_def=1)


def test_fused_squeezenet_with_its_feed_resized(lite, wl, plref, squeezenet, img224, ref224):
    """The program lowered with L for batch 2 runs with its feed resized to one image (every kernel class reads its dims in Run),
    and back at batch 2 reproduces its first result."""
    img1 = np.random.default_rng(353).uniform(-1, 1, (1, 3, 224, 224)).astype(F32)
    ref1 = _ref(plref, squeezenet, img1, "pool10")
    p, out, plan = _run(lite, wl, squeezenet, img224, fuse=True)
    assert len([l for l in plan if l.startswith("concat/int8 ")]) == 8
    try:
        dev_out = out[:-len("/host")]
        first = p.get_var(dev_out, F32)
        np.testing.assert_allclose(first, ref224[dev_out], rtol=1e-5, atol=1e-5)
        survive = sorted(n for n in _written(plan) if n in ref1)
        p.add_feed(squeezenet["input"], img1.shape, lite.PREC_FLOAT)
        p.set_input(squeezenet["input"], img1)
        p.run()
        for name in survive:
            _check(p, name, ref1[name])
        p.add_feed(squeezenet["input"], img224.shape, lite.PREC_FLOAT)
        p.set_input(squeezenet["input"], img224)
        p.run()
        assert np.array_equal(p.get_var(dev_out, F32), first)
    finally:
        p.close()
