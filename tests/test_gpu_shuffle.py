"""-m gpu: concat / split / shuffle_channel and the one-launch unit tail on the device.  The four C ABI calls against the numpy
restatements of shuffle_oracle.py (fp32 compared as uint32: values are moved, NaN payloads and -0.0 included; int8 against calib's
restatement and against plhip_calib_f32_to_i8), with aligned bases and bases off by one element; the kernel classes through
KernelFactory -> SetParam -> Launch; ShuffleNetV2 whole programs against the helper oracle, unfused and with fusion K."""
import ctypes as C
import importlib

import numpy as np
import pytest

import shuffle_oracle as S

pytestmark = pytest.mark.gpu
F32 = np.float32
SCALE = 4.0 / 127


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = _bits(got), _bits(want)
    assert np.array_equal(g, w), "%s: %d of %d fp32 values differ in their bits" % (what, (g != w).sum(), w.size)


def _same_i8(gpu_ctx, got_q, want_f32, what):
    """The restatement of calib wherever the value is a number; everywhere (NaN included) what plhip_calib_f32_to_i8 makes of it."""
    assert got_q.shape == want_f32.shape, what
    num = ~np.isnan(want_f32)
    want_q = S.calib_i8(want_f32, SCALE)
    assert np.array_equal(got_q[num], want_q[num]), "%s: %d int8 values differ from the oracle" % (what, (got_q[num] != want_q[num]).sum())
    if want_f32.size:
        assert np.array_equal(got_q, gpu_ctx.calib_f32_to_i8(want_f32, SCALE)), what + ": differs from the separate calib call"


def _inputs(rng, shape):
    """randn * 4 with NaN (two payloads), +-inf, +-0, denormals and +-3e38 planted."""
    x = (rng.standard_normal(shape) * 4).astype(F32)
    edge = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38, 126.5 * SCALE, -0.5 * SCALE], F32)
    flat = x.reshape(-1)
    k = min(flat.size, edge.size)
    pos = rng.permutation(flat.size)[:k]
    flat[pos] = edge[:k]
    flat.view(np.uint32)[pos[0]] = 0x7FC12345  # the NaN carries a payload of its own
    return x


CONCAT_CASES = [(1, [1, 1], 1), (3, [2, 5], 49), (2, [58, 58], 196), (2, [24, 24, 24], 16), (2, [3, 1, 4, 2], 7), (1, [1] * 9, 5),
                (1, [2, 3], 120), (6, [2, 3], 1)]


@pytest.mark.parametrize("outer,cs,inner", CONCAT_CASES)
def test_concat_and_split_move_bits(gpu_ctx, outer, cs, inner):
    rng = np.random.default_rng(400 + outer + inner + len(cs))
    if (outer, inner) == (1, 120):      # axis 0
        xs, axis = [_inputs(rng, (c, inner)) for c in cs], 0
    elif inner == 1:                    # the last axis
        xs, axis = [_inputs(rng, (outer, c)) for c in cs], 1
    else:
        xs, axis = [_inputs(rng, (outer, c, inner)) for c in cs], 1
    want = S.concat(xs, axis)
    for mis in (0, 1):
        y = gpu_ctx.concat(xs, axis, misalign=mis)
        _same_bits(y, want, "concat %s misalign %d" % ((outer, cs, inner), mis))
        parts = gpu_ctx.split(want, axis, sections=cs, misalign=mis)
        ref_parts = S.split(want, axis, sections=cs)
        assert len(parts) == len(cs)
        for i, (p, r, x) in enumerate(zip(parts, ref_parts, xs)):
            _same_bits(p, r, "split %s part %d misalign %d" % ((outer, cs, inner), i, mis))
            _same_bits(p, x, "split of concat, part %d" % i)
        if len(set(cs)) == 1:
            for p, x in zip(gpu_ctx.split(want, axis, num=len(cs), misalign=mis), xs):
                _same_bits(p, x, "split num=%d misalign %d" % (len(cs), mis))


@pytest.mark.parametrize("n,c,hw,group", [(1, 2, 1, 2), (3, 6, 49, 3), (2, 58, 49, 2), (2, 116, 196, 2), (2, 48, 64, 4), (1, 24, 784, 8)])
def test_shuffle_channel_bit_exact(gpu_ctx, n, c, hw, group):
    rng = np.random.default_rng(410 + c + hw)
    x = _inputs(rng, (n, c, hw))
    want = S.shuffle_channel(x, group)
    for mis in (0, 1):
        what = "shuffle_channel %s misalign %d" % ((n, c, hw, group), mis)
        yf, _ = gpu_ctx.shuffle_channel(x, group, mode="f32", misalign=mis)
        _, yq = gpu_ctx.shuffle_channel(x, group, mode="i8", calib_scale=SCALE, misalign=mis)
        bf, bq = gpu_ctx.shuffle_channel(x, group, mode="both", calib_scale=SCALE, misalign=mis)
        _same_bits(yf, want, what)
        _same_i8(gpu_ctx, yq, want, what)
        _same_bits(bf, want, what + " (both)")
        assert np.array_equal(bq, yq), what


@pytest.mark.parametrize("n,h,hw,split_at", [(1, 1, 1, 1), (3, 3, 49, 3), (2, 58, 49, 58), (2, 58, 196, 58), (2, 24, 784, 24), (2, 29, 196, 0),
                                             (2, 116, 49, 0), (1, 5, 12, 7)])
def test_shuffle_unit_equals_the_oracle_and_the_four_calls(gpu_ctx, n, h, hw, split_at):
    rng = np.random.default_rng(420 + h + hw + split_at)
    a, b = _inputs(rng, (n, h, hw)), _inputs(rng, (n, h, hw))
    lo_w, hi_w, _ = S.shuffle_unit(a, b, split_at)
    # the four separate C ABI calls: concat -> shuffle_channel -> split -> calib
    cat = gpu_ctx.concat([a, b], 1)
    shuf, _ = gpu_ctx.shuffle_channel(cat, 2)
    if split_at == 0:
        lo_s, hi_s = None, shuf
    else:
        lo_s, hi_s = gpu_ctx.split(shuf, 1, sections=(split_at, 2 * h - split_at))
    q_s = gpu_ctx.calib_f32_to_i8(hi_s, SCALE)
    _same_bits(hi_s, hi_w, "the separate calls, second part")
    for mis in (0, 1):
        what = "unit %s misalign %d" % ((n, h, hw, split_at), mis)
        lo, hf, _ = gpu_ctx.shuffle_unit(a, b, split_at, mode="f32", misalign=mis)
        lo2, _, hq = gpu_ctx.shuffle_unit(a, b, split_at, mode="i8", calib_scale=SCALE, misalign=mis)
        lo3, bf, bq = gpu_ctx.shuffle_unit(a, b, split_at, mode="both", calib_scale=SCALE, misalign=mis)
        if split_at == 0:
            assert lo is None and lo2 is None and lo3 is None
        else:
            for l in (lo, lo2, lo3):
                _same_bits(l, lo_w, what + " lo")
                assert l.tobytes() == lo_s.tobytes(), what
        _same_bits(hf, hi_w, what + " hi")
        _same_bits(bf, hi_w, what + " hi (both)")
        assert hf.tobytes() == hi_s.tobytes() and bf.tobytes() == hi_s.tobytes(), what
        _same_i8(gpu_ctx, hq, hi_w, what)
        assert hq.tobytes() == q_s.tobytes() and bq.tobytes() == q_s.tobytes(), what


def test_bad_arguments_are_refused(gpu_ctx, pkg):
    L = pkg.capi.load()
    with gpu_ctx.scope() as s:
        d = s.alloc(4096)
        h = gpu_ctx.h
        null = C.c_void_p()
        two = (C.c_void_p * 2)(d, d)
        one_null = (C.c_void_p * 2)(d, null)

        def ext(*v):
            return (C.c_int64 * len(v))(*v)
        assert L.plhip_concat_f32(h, two, ext(2, 3), 2, 1, 4, d) == 0
        assert L.plhip_concat_f32(h, two, ext(2, 3), 2, 1, 4, null) < 0        # null output
        assert L.plhip_concat_f32(h, one_null, ext(2, 3), 2, 1, 4, d) < 0      # a null input
        assert L.plhip_concat_f32(h, two, ext(2, 0), 2, 1, 4, d) < 0           # an extent < 1
        assert L.plhip_concat_f32(h, two, ext(2, 3), 0, 1, 4, d) < 0           # no inputs
        assert L.plhip_concat_f32(h, two, ext(2, 3), 2, 0, 4, d) < 0
        assert L.plhip_concat_f32(h, two, ext(1 << 30, 1 << 30), 2, 1 << 30, 4, d) < 0   # outer * sum * inner beyond 2^40 elements
        assert L.plhip_concat_f32(h, two, ext(1 << 39, 1 << 39), 2, 1, 4, d) < 0
        assert L.plhip_split_f32(h, d, 1 << 20, 1 << 20, 1 << 20, 2, None, 2, two) < 0
        assert L.plhip_split_f32(h, d, 1, 6, 4, 2, None, 2, two) == 0
        assert L.plhip_split_f32(h, d, 1, 6, 4, 0, ext(2, 4), 2, two) == 0
        assert L.plhip_split_f32(h, d, 1, 7, 4, 2, None, 2, two) < 0           # num does not divide the axis
        assert L.plhip_split_f32(h, d, 1, 6, 4, 3, None, 2, two) < 0           # num != count
        assert L.plhip_split_f32(h, d, 1, 6, 4, 0, ext(2, 3), 2, two) < 0      # sections do not add up
        assert L.plhip_split_f32(h, d, 1, 6, 4, 0, None, 2, two) < 0           # neither num nor sections
        assert L.plhip_split_f32(h, d, 1, 6, 4, 2, None, 2, one_null) < 0      # a null output
        assert L.plhip_shuffle_channel_f32(h, d, 1, 6, 4, 3, d, null, 1.0) == 0
        assert L.plhip_shuffle_channel_f32(h, d, 1, 6, 4, 4, d, null, 1.0) < 0     # group does not divide c
        assert L.plhip_shuffle_channel_f32(h, d, 1, 6, 4, 3, null, null, 1.0) < 0  # no output
        assert L.plhip_shuffle_channel_f32(h, d, 1, 6, 4, 3, null, d, 0.0) < 0     # int8 output without a positive scale
        assert L.plhip_shuffle_channel_f32(h, null, 1, 6, 4, 3, d, null, 1.0) < 0
        assert L.plhip_shuffle_unit_f32(h, d, d, 1, 3, 4, 3, d, d, null, 1.0) == 0
        assert L.plhip_shuffle_unit_f32(h, d, d, 1, 3, 4, 3, null, d, null, 1.0) < 0   # lo_f32 null with split_at > 0
        assert L.plhip_shuffle_unit_f32(h, d, d, 1, 3, 4, 0, d, d, null, 1.0) < 0      # lo_f32 given with split_at == 0
        assert L.plhip_shuffle_unit_f32(h, d, d, 1, 3, 4, 7, d, d, null, 1.0) < 0      # split_at > 2 h
        assert L.plhip_shuffle_unit_f32(h, d, d, 1, 3, 4, -1, d, d, null, 1.0) < 0
        assert L.plhip_shuffle_unit_f32(h, d, d, 1, 3, 4, 3, d, null, null, 1.0) < 0   # nothing for the second part
        assert L.plhip_shuffle_unit_f32(h, d, d, 1, 3, 4, 3, d, null, d, 0.0) < 0      # int8 without a positive scale
        assert L.plhip_shuffle_unit_f32(h, d, null, 1, 3, 4, 3, d, d, null, 1.0) < 0
        assert L.plhip_shuffle_unit_f32(h, d, d, 1, 3, 4, 6, d, null, null, 1.0) == 0  # everything below split_at: no second part
        gpu_ctx.sync()


def test_kernel_classes_through_the_factory(lite):
    rng = np.random.default_rng(430)
    a, b = _inputs(rng, (2, 6, 5, 7)), _inputs(rng, (2, 6, 5, 7))
    p = lite.Predictor(0)
    try:
        for name, v in (("a", a), ("b", b)):
            p.add_feed(name, v.shape)
            p.add_io_copy(name, name + "d", True)
        p.add_concat(["ad", "bd", "ad"], "cat3", 1)
        p.add_concat(["ad", "bd"], "cat", 1)
        p.add_shuffle_channel("cat3", "sh3", 3)
        p.add_shuffle_channel("cat", "sh", 2)
        p.add_split("sh", ["lo", "hi"], 1, 2)
        p.add_split("cat3", ["p0", "p1", "p2"], -3, 0, (5, 1, 12))
        p.add_shuffle_unit("ad", "bd", "", "k2", "k2_q", SCALE, False)
        p.add_shuffle_unit("ad", "bd", "", "k2d", "k2d_q", SCALE, True)
        p.add_shuffle_unit("ad", "bd", "ulo", "uhi", "uhi_q", SCALE, True)
        p.add_shuffle_unit("ad", "bd", "vlo", "vhi", "vhi_q", SCALE, False)
        p.set_input("a", a)
        p.set_input("b", b)
        p.run()
        p.run()
        names = "\n".join(p.kernel_names())
        for frag in ("/def -> concat_hip", "/def -> split_hip", "/def -> shuffle_channel_hip", "/int8 -> shuffle_concat_fp32_int8_hip",
                     "/int8 -> shuffle_concat_int8_hip", "/unit -> shuffle_unit_int8_hip", "/unit -> shuffle_unit_fp32_int8_hip"):
            assert frag in names, (frag, names)
        cat3, cat = S.concat([a, b, a], 1), S.concat([a, b], 1)
        sh = S.shuffle_channel(cat, 2)
        _same_bits(p.get_var("cat3", F32), cat3, "concat class")
        _same_bits(p.get_var("sh3", F32), S.shuffle_channel(cat3, 3), "shuffle_channel class")
        _same_bits(p.get_var("lo", F32), sh[:, :6], "split class, num")
        _same_bits(p.get_var("hi", F32), sh[:, 6:], "split class, num")
        for name, want in zip(("p0", "p1", "p2"), S.split(cat3, 1, sections=(5, 1, 12))):
            _same_bits(p.get_var(name, F32), want, "split class, sections")
        _same_bits(p.get_var("k2", F32), sh, "shuffle_channel/int8, fp32 output")
        q = p.get_var("k2_q", np.int8)
        num = ~np.isnan(sh)
        assert q.shape == sh.shape and np.array_equal(q[num], S.calib_i8(sh, SCALE)[num])
        assert np.array_equal(p.get_var("k2d_q", np.int8), q)
        for lo, hi, hq in (("ulo", None, "uhi_q"), ("vlo", "vhi", "vhi_q")):
            _same_bits(p.get_var(lo, F32), sh[:, :6], "shuffle_channel/unit lo")
            assert np.array_equal(p.get_var(hq, np.int8), q[:, 6:])
            if hi:
                _same_bits(p.get_var(hi, F32), sh[:, 6:], "shuffle_channel/unit hi")
    finally:
        p.close()


# ------------------------------------------------------------------ whole programs
def _run(lite, wl, net, img, **kw):
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, img.shape[0], **kw)
        plan = p.graph_plan()
        assert p.graph_lower() == [out]
        p.set_input(net["input"], img)
        p.run()
        p.run()
        return p, out, plan
    except Exception:
        p.close()
        raise


def _written(plan):
    """The device variables a plan writes, read off its lines: every out= (not behind -f32, not the host copy), +hi=, +calib=."""
    names = set()
    for l in plan:
        toks = l.split(" ")
        kv = dict(f.split("=", 1) for f in toks[1:] if "=" in f)
        if l.startswith("io_copy/device_to_host"):
            continue
        if "-f32" not in toks:
            names.update(kv["out"].split(","))
        for k in ("+calib", "+hi"):
            if k in kv:
                names.add(kv[k])
    return names


def _pooled(ref):
    return {k: v.reshape(v.shape[0], -1, 1, 1) if k == "pool" else v for k, v in ref.items()}


def _check(p, name, want):
    got = p.get_var(name, want.dtype)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if want.dtype == np.int8:
        assert np.array_equal(got, want), "%s: %d of %d int8 values differ" % (name, (got != want).sum(), want.size)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5, err_msg=name)


@pytest.fixture(scope="module")
def net10(wl):
    return wl.shufflenet_v2_net(1.0)


@pytest.fixture(scope="module")
def img10():
    return np.random.default_rng(350).uniform(-1, 1, (2, 3, 224, 224)).astype(F32)


@pytest.fixture(scope="module")
def ref10(plref, net10, img10):
    return _pooled(S.forward(plref, net10, img10))


def _program_case(lite, wl, net, img, ref):
    pu, out, plan_u = _run(lite, wl, net, img, fuse=False)
    try:
        names = "\n".join(pu.kernel_names())
        assert names.count("concat_hip") == 16 and names.count("shuffle_channel_hip") == 16 and names.count("split_hip") == 13
        assert {n for n in _written(plan_u) if "/target_trans" not in n} == set(ref)
        for name, want in ref.items():
            _check(pu, name, want)
        # the three ops move values: their outputs hold the bits of the device's own inputs
        for o in net["ops"]:
            if o["op"] == "concat":
                _same_bits(pu.get_var(o["name"], F32), S.concat([pu.get_var(v, F32) for v in o["srcs"]], 1), o["name"])
            elif o["op"] == "shuffle_channel":
                _same_bits(pu.get_var(o["name"], F32), S.shuffle_channel(pu.get_var(o["src"], F32), o["group"]), o["name"])
            elif o["op"] == "split":
                for nm, want in zip(o["names"], S.split(pu.get_var(o["src"], F32), 1, num=2)):
                    _same_bits(pu.get_var(nm, F32), want, nm)
        pf, outf, plan_f = _run(lite, wl, net, img, fuse=True, fuse_shuffle=True)
        try:
            fnames = "\n".join(pf.kernel_names())
            assert fnames.count("shuffle_unit_int8_hip") == 13 and fnames.count("shuffle_concat_int8_hip") == 3
            assert not [k for k in ("concat_hip", "split_hip", "shuffle_channel_hip") if k in fnames]
            p_off = lite.Predictor(planner=True)
            try:
                wl.emit_graph(p_off, net, img.shape[0], fuse=True, fuse_shuffle=False)
                assert len(p_off.graph_plan()) - len(plan_f) == 45 and pf.num_instructions() == len(plan_f)
            finally:
                p_off.close()
            survive = sorted(n for n in _written(plan_f) if n in ref)
            gone = set(ref) - set(survive)
            assert {n for n in gone if n.endswith(("_concat", "_shuffle", "_x2"))} == {o["name"] for o in net["ops"] if o["op"] in ("concat", "shuffle_channel")} | \
                {o["names"][1] for o in net["ops"] if o["op"] == "split"}
            assert all(n in survive for n in ref if n.endswith(("_x1", "_x2/precision_trans", "_shuffle/precision_trans")))
            assert len(survive) > len(ref) // 2
            for name in survive:
                want = ref[name]
                got = pf.get_var(name, want.dtype)
                assert got.shape == want.shape, name
                assert np.array_equal(got.view(np.uint8), pu.get_var(name, want.dtype).view(np.uint8)), name
        finally:
            pf.close()
    finally:
        pu.close()


def test_shufflenet_v2_1_0_program_vs_oracle(lite, wl, net10, img10, ref10):
    """scale 1.0, 224 x 224, batch 2: 7 x 7 planes (the scalar path) and 58-channel halves.  Unfused: every variable, int8 bit for
    bit, fp32 within rtol 1e-5; with K: every surviving variable byte for byte what the unfused GPU run wrote."""
    _program_case(lite, wl, net10, img10, ref10)


def test_shufflenet_v2_0_5_program_vs_oracle(lite, wl, plref):
    """scale 0.5, 96 x 96, batch 3: planes 12 x 12, 6 x 6 and 3 x 3."""
    net = wl.shufflenet_v2_net(0.5, res=96)
    assert [net["shapes"]["s%du1_shuffle" % s][1:] for s in (2, 3, 4)] == [(12, 12), (6, 6), (3, 3)]
    img = np.random.default_rng(351).uniform(-1, 1, (3, 3, 96, 96)).astype(F32)
    _program_case(lite, wl, net, img, _pooled(S.forward(plref, net, img)))


def test_fused_program_with_its_feed_resized(lite, wl, plref, net10, img10, ref10):
    """The program lowered with K for 224 x 224 runs with its feed resized to 192 x 192 (every kernel class reads its dims in Run),
    and back at 224 reproduces its first result."""
    net192 = wl.shufflenet_v2_net(1.0, res=192)
    img192 = np.random.default_rng(352).uniform(-1, 1, (2, 3, 192, 192)).astype(F32)
    ref192 = _pooled(S.forward(plref, net192, img192))
    p, out, plan = _run(lite, wl, net10, img10, fuse=True, fuse_shuffle=True)
    try:
        dev_out = out[:-len("/host")]
        first = p.get_var(dev_out, F32)
        np.testing.assert_allclose(first, ref10[dev_out], rtol=1e-5, atol=1e-5)
        survive = sorted(n for n in _written(plan) if n in ref192)
        p.add_feed(net10["input"], img192.shape, lite.PREC_FLOAT)
        p.set_input(net10["input"], img192)
        p.run()
        for name in survive:
            _check(p, name, ref192[name])
        p.add_feed(net10["input"], img10.shape, lite.PREC_FLOAT)
        p.set_input(net10["input"], img10)
        p.run()
        assert np.array_equal(p.get_var(dev_out, F32), first)
    finally:
        p.close()
