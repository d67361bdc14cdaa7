"""CPU tests of fusion L and the networks it is for: the exported symbols and the registered kernel, the kernel class against the
reference's ConcatParam text, the structure and the health of squeezenet_v1_1_net and inception_mini_net, their lowering
(unfused: the reference's instruction list; fused: rule L restated here over the L-off plan; the exact lines recorded under
tests/golden/concat_plans/), the graphs where L must and must not fire, and the kept ISA of the new kernel."""
import ctypes as C
import glob
import importlib
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import shuffle_oracle as S

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITE = os.path.join(ROOT, "paddle-lite_amd")


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


@pytest.fixture(scope="module")
def squeezenet(wl):
    return wl.squeezenet_v1_1_net()


@pytest.fixture(scope="module")
def inception(wl):
    return wl.inception_mini_net()


# ------------------------------------------------------------------ exports, registration, structs
def test_new_symbols_are_exported_and_the_kernel_registered(pkg, lite):
    capi = pkg.capi
    L = capi.load()
    assert "plhip_concat_calib_f32" in capi.EXPORTS and hasattr(L, "plhip_concat_calib_f32")
    LL = lite.load()
    for name in ("pllite_graph_set_fuse_concat", "pllite_add_concat_calib"):
        assert hasattr(LL, name), name
    for name in ("graph_set_fuse_concat", "add_concat_calib"):
        assert hasattr(lite.Predictor, name), name
    # concat/int8 reads fp32 and writes int8: it is registered at kAny precision, and concat/def stays the one kernel at kFloat
    assert LL.pllite_registered_kernels(b"concat", lite.PREC_ANY, lite.LAYOUT_NCHW) == 1
    assert LL.pllite_registered_kernels(b"concat", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1
    src = open(os.path.join(LITE, "lite", "kernels", "hip", "shuffle_compute.cc")).read()
    assert re.findall(r"REGISTER_LITE_KERNEL\(concat, kHIP, (\w+), kNCHW, [\w:]+, (\w+)\)", src) == [("kFloat", "def"), ("kAny", "int8")]


@pytest.mark.skipif(not os.path.isdir("/root/reference/lite"), reason="reference tree not present on this machine")
def test_concat_calib_compute_compiles_against_the_reference_param_struct():
    """The method of test_boundary_reference_params.py: the generated header holds the reference's own struct text, and the fusion
    state lives in the side header."""
    with tempfile.TemporaryDirectory(prefix="khip_refparams.") as tmp:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_ref_params_header.py"), "--out", tmp], stdout=subprocess.DEVNULL)
        gen = open(os.path.join(tmp, "lite", "operators", "op_params.h")).read()
        assert "struct ConcatParam" in gen and "calib_output" not in gen and "drop_fp32_output" not in gen
        side = open(os.path.join(LITE, "lite", "kernels", "hip", "calib_tail.h")).read()
        assert "calib_output" in side and "calib_scale" in side and "drop_fp32_output" in side
        p = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", tmp, "-I", LITE, "-I", os.path.join(ROOT, "include"),
                            os.path.join(LITE, "lite", "kernels", "hip", "shuffle_compute.cc")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "shuffle_compute.cc does not compile against the reference's structs:\n%s" % p.stdout.decode()[-3000:]


# ------------------------------------------------------------------ structure
def test_structure_of_both_generators(wl, squeezenet, inception, pkg):
    ops, sh = squeezenet["ops"], squeezenet["shapes"]
    assert sum(o["op"] == "concat" for o in ops) == 8 and sum(o["op"] == "conv2d" for o in ops) == 26
    assert [o["name"] for o in ops if o["op"] == "pool2d"] == ["pool1", "pool3", "pool5", "pool10"]
    assert sh["conv1"] == (64, 112, 112) and sh["pool1"] == (64, 55, 55) and sh["pool3"] == (128, 27, 27) and sh["pool5"] == (256, 13, 13)
    assert [sh["fire%d_concat" % i] for i in range(2, 10)] == [(128, 55, 55), (128, 55, 55), (256, 27, 27), (256, 27, 27), (384, 13, 13),
                                                               (384, 13, 13), (512, 13, 13), (512, 13, 13)]
    assert [sh["fire%d_squeeze" % i][0] for i in range(2, 10)] == [16, 16, 32, 32, 48, 48, 64, 64]
    assert sh["conv10"] == (1000, 13, 13) and sh["prob"] == (1000, 1, 1)
    assert sum(np.prod(sh["fire%d_concat" % i]) for i in range(2, 10)) == 1450496  # concatenated elements per image
    assert wl.concat_calib_bytes(squeezenet, 128) == (17 * 128 * 1450496, 9 * 128 * 1450496)
    for o in ops:
        if o["op"] == "concat":
            assert o["axis"] == 1 and len(o["srcs"]) == 2
    assert wl.squeezenet_v1_1_net(res=96, num_classes=10)["shapes"]["conv10"] == (10, 5, 5)
    ops, sh = inception["ops"], inception["shapes"]
    assert sum(o["op"] == "concat" for o in ops) == 2 and all(len(o["srcs"]) == 4 for o in ops if o["op"] == "concat")
    assert sh["conv1"] == (32, 32, 32) and sh["conv2"] == (64, 32, 32)
    assert sh["inc1_concat"] == (16 + 32 + 8 + 8, 32, 32) and sh["inc2_concat"] == (32 + 48 + 24 + 16, 32, 32)
    assert sh["inc1_pool"] == (64, 32, 32) and sh["inc2_pool"] == (64, 32, 32) and sh["inc2_5x5_reduce"] == (8, 32, 32)
    assert sh["fc"] == (10, 1, 1) and sh["prob"] == (10, 1, 1)
    # the conv routes SqueezeNet's new shapes take (1x1 with K = 16 on a 3025-pixel plane, 3x3 with Cin = 16 / 48, 512 -> 1000 at 13 x 13)
    capi = pkg.capi
    L = capi.load()
    full = dict(squeezenet["shapes"], image=squeezenet["input_shape"])
    for o in squeezenet["ops"]:
        if o["op"] == "conv2d":
            cin, h, w = full[o["src"]]
            cout, _, k, _ = o["w"].shape
            d = capi.conv_desc(2, cin, h, w, cout, k, k, (o["pad"],) * 4, (o["stride"],) * 2, (1, 1), 1, act=capi.ACT_RELU)
            impl = L.plhip_conv_impl_name(C.byref(d)).decode()
            print("%-18s %4d -> %4d k%d s%d @%dx%d: %s" % (o["name"], cin, cout, k, o["stride"], h, w, impl))
            assert impl and impl != "unsupported", o["name"]


# ------------------------------------------------------------------ health, on the oracle alone
def _shares(ref):
    """name -> (share of values at +-127, share of zeros) of every int8 activation tensor."""
    return {k: ((np.abs(v.astype(np.int32)) == 127).mean(), (v == 0).mean()) for k, v in ref.items() if v.dtype == np.int8}


def test_both_networks_are_as_healthy_as_mobilenet_v2(wl, plref, squeezenet, inception):
    """The rule of test_synthetic_network_is_as_healthy_as_mobilenet_v2: the yardstick is computed here, not written down, from
    the worst int8 tensor of mobilenet_v2_net on the same images (0.048 saturated, 0.637 zeros when this was written).  Measured:
    SqueezeNet v1.1 0.045 / 0.548 over 18 tensors; the inception net 0.029 / 0.613 over 11 (its worst saturated share is the pooled
    tensor in front of the fc, 240 values; every other tensor is at or below 0.012)."""
    import oracle.graph_oracle as GO
    img = np.random.default_rng(350).uniform(-1, 1, (2, 3, 224, 224)).astype(F32)
    mb = _shares(GO.forward(plref, wl.mobilenet_v2_net(), img, via_gemm=True))
    worst_sat, worst_zero = max(v[0] for v in mb.values()), max(v[1] for v in mb.values())
    assert 0 < worst_sat < 0.1 and 0.5 < worst_zero < 0.8
    img64 = np.random.default_rng(350).uniform(-1, 1, (2, 3, 64, 64)).astype(F32)
    for tag, net, x, n_int8, classes in (("squeezenet_v1_1", squeezenet, img, 18, (2, 1000, 1, 1)), ("inception_mini", inception, img64, 11, (2, 10))):
        ref = S.forward(plref, net, x, via_gemm=True)
        sh = _shares(ref)
        assert len(sh) == n_int8, sorted(sh)
        print("%s: worst saturated %.4f (yardstick %.4f), worst zero %.4f (yardstick %.4f)" % (
            tag, max(v[0] for v in sh.values()), worst_sat, max(v[1] for v in sh.values()), worst_zero))
        for name, (sat, zero) in sh.items():
            assert sat <= worst_sat, (tag, name, sat, worst_sat)
            assert zero <= worst_zero, (tag, name, zero, worst_zero)
        assert ref["prob"].shape == classes and np.isfinite(ref["prob"]).all()
        if tag == "squeezenet_v1_1":  # softmax runs along the last axis of [N, C, 1, 1]: the network's result is the pooled tensor
            assert np.isfinite(ref["pool10"]).all() and ref["pool10"].std() > 0


# ------------------------------------------------------------------ plans
def _plan(lite, wl, net, batch=2, **kw):
    p = lite.Predictor(planner=True)
    try:
        wl.emit_graph(p, net, batch, **kw)
        return p.graph_plan()
    finally:
        p.close()


def _heads(plan):
    return [l.split(" ")[0] for l in plan]


def _kv(line):
    return dict(f.split("=", 1) for f in line.split(" ")[1:] if "=" in f)


def _rule_l(plan, net):
    """Rule L restated over a plan that was made without it.  Returns (new plan, concats with a direct calib, concats without)."""
    ops = {o["name"]: o for o in net["ops"]}
    lines = list(plan)
    dead = set()

    def readers(v):
        return [j for j, l in enumerate(lines) if j not in dead and (v in _kv(l)["in"].split(",") or _kv(l).get("+add") == v)]

    l1, l2_only = [], []
    for i, line in enumerate(plan):
        if not line.startswith("concat/def "):
            continue
        kv = _kv(line)
        out = kv["out"]
        direct = [j for j in readers(out) if lines[j].startswith("calib/fp32_to_int8 ")]
        assert len(direct) <= 1
        pools = []
        for j in readers(out):
            if not lines[j].startswith("pool2d/def ") or lines[j].endswith(" int8"):
                continue
            o = ops[_kv(lines[j])["out"]]
            if o["pooling_type"] != "max" or o["global_pooling"]:
                continue
            r = readers(_kv(lines[j])["out"])
            if len(r) == 1 and lines[r[0]].startswith("calib/fp32_to_int8 "):
                pools.append((j, r[0]))
        scales = {_kv(lines[c])["scale"] for _, c in pools}  # the %.9g text of a float32 names its bits
        if direct:
            scale, q = _kv(lines[direct[0]])["scale"], _kv(lines[direct[0]])["out"]
            dead.add(direct[0])
            l1.append(out)
        elif pools and len(scales) == 1:
            scale, q = scales.pop(), out + "/precision_trans"
            l2_only.append(out)
        else:
            continue
        for j, c in pools:
            if _kv(lines[c])["scale"] == scale:
                lines[j] = "pool2d/def in=%s out=%s int8" % (q, _kv(lines[c])["out"])
                dead.add(c)
        lines[i] = "concat/int8 in=%s out=%s +calib=%s scale=%s%s axis=%s" % (kv["in"], out, q, scale, "" if readers(out) else " -f32", kv["axis"])
    return [l for j, l in enumerate(lines) if j not in dead], l1, l2_only


def _check_unfused(plan, net):
    want = S.plan(net)
    body = plan[1:-1]
    assert len(body) == len(want)
    for line, (kind, s) in zip(body, want):
        head, toks = line.split(" ")[0], line.split(" ")
        if kind == "calib":
            src = s["src"] + ("/target_trans" if s["src"] == net["input"] else "")
            assert head == "calib/fp32_to_int8" and ("in=" + src) in toks and ("out=" + s["dst"]) in toks, line
            continue
        o = s["o"]
        if o["op"] in S.INT8_OPS:
            alias = ("int8out" if s["int8_out"] else "fp32out") if o["op"] == "fc" else ("int8_out" if s["int8_out"] else "fp32_out")
        else:
            alias = "def"
        assert head == o["op"] + "/" + alias, line
        assert ("in=" + ",".join(s["ins"])) in toks and ("out=" + o["name"]) in toks, line


def test_lowering_of_both_networks(lite, wl, squeezenet, inception):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dump_concat_plans as D
    golden = D.load_fixtures()
    assert len(golden) == 8
    for tag, net in (("squeezenet_v1_1", squeezenet), ("inception_mini", inception)):
        nofuse = _plan(lite, wl, net, fuse=False)
        _check_unfused(nofuse, net)
        off = _plan(lite, wl, net, fuse=True, fuse_concat=False)
        on = _plan(lite, wl, net, fuse=True, fuse_concat=True)
        default = _plan(lite, wl, net, fuse=True)
        assert not [h for h in _heads(off) if h == "concat/int8"]
        want, l1, l2_only = _rule_l(off, net)
        assert on == want
        assert default == on        # L is on by default (measured)
        assert _plan(lite, wl, net, fuse=False, fuse_concat=True) == nofuse     # L needs set_fuse(true)
        for sw, got in (("nofuse", nofuse), ("default", default), ("concat_off", off), ("concat_on", on)):
            assert got == golden["%s.%s.b2" % (tag, sw)], (tag, sw)
        for pl in (nofuse, off, on):
            costs = wl.program_costs(net, 2, pl)
            assert len(costs) == len(pl) and all(c["bytes"] >= 0 for c in costs)
        if tag == "squeezenet_v1_1":
            # six concats have a calib of their own (fire2, 4, 6, 7, 8: the next squeeze conv; fire9: conv10), the two in front of a max
            # pool (fire3, fire5) only the pool's; no fp32 concat tensor is written any more and both pools run on int8
            assert l1 == ["fire%d_concat" % i for i in (2, 4, 6, 7, 8, 9)] and l2_only == ["fire3_concat", "fire5_concat"]
            cats = [l for l in on if l.startswith("concat/")]
            assert len(cats) == 8 and all(l.startswith("concat/int8 ") and " -f32 " in l for l in cats)
            assert "pool2d/def in=fire3_concat/precision_trans out=pool3/precision_trans int8" in on
            assert "pool2d/def in=fire5_concat/precision_trans out=pool5/precision_trans int8" in on
            assert len(off) - len(on) == 8
            moved = lambda pl: sum(c["bytes"] for c, l in zip(wl.program_costs(net, 2, pl), pl) if l.startswith(("concat/", "calib/fp32_to_int8 in=fire")))
            n = 2 * 1450496
            assert moved(on) == 5 * n    # the operands once, the int8 tensor once
        else:
            assert l1 == ["inc1_concat"] and l2_only == []
            assert [l for l in on if l.startswith("concat/")] == [
                "concat/int8 in=inc1_1x1,inc1_3x3,inc1_5x5,inc1_pool_proj out=inc1_concat +calib=inc1_concat/precision_trans scale=0.0472440943 -f32 axis=1",
                "concat/def in=inc2_1x1,inc2_3x3,inc2_5x5,inc2_pool_proj out=inc2_concat axis=1"]
            assert "pool2d/def in=inc1_concat/precision_trans out=inc2_pool/precision_trans int8" in on
            assert "pool2d/def in=conv2 out=inc1_pool" in on          # the first block's pool reads a conv: fp32
            assert "pool2d/def in=inc2_concat out=pool" in on         # the global average pool behind the last concat
            assert len(off) - len(on) == 2


# ------------------------------------------------------------------ mini graphs where L must and must not fire
def _mini(lite, build, fetch=("out",), fuse=True, fuse_concat=True):
    """A planner graph: feed x [2, 8, 4, 4] -> build(p) -> the fetches."""
    p = lite.Predictor(planner=True)
    try:
        p.graph_set_fuse(fuse)
        if fuse_concat is not None:
            p.graph_set_fuse_concat(fuse_concat)
        p.graph_feed("x", (2, 8, 4, 4))
        build(p)
        for f in fetch:
            p.graph_fetch(f)
        return p.graph_plan()
    finally:
        p.close()


def _conv(p, src, dst, cin, cout, in_scale=0.05):
    w = np.ones((cout, cin, 1, 1), np.int8)
    p.graph_conv("conv2d", src, dst, w, None, (1, 1), (0, 0, 0, 0), (1, 1), 1, 1, 0.0, in_scale, np.full(cout, 0.01, F32))


def _pool(p, src, dst, kind="max", global_pooling=False):
    p.graph_pool(src, dst, kind, (2, 2), (2, 2), (0, 0, 0, 0), global_pooling, True, False)


def _cat(p, n_in=2, axis=1):
    names = ["a", "b", "c"][:n_in]
    for v in names:
        _conv(p, "x", v, 8, 8)
    p.graph_concat(names, "cat", axis)
    return 8 * n_in if axis == 1 else 8


S05, S07 = "0.0500000007", "0.0700000003"


def test_fusion_l_fires_only_on_its_pattern(lite):
    def cats(plan):
        return [l for l in plan if l.startswith(("concat/", "pool2d/", "shuffle_channel/")) or (l.startswith("calib/") and "in=x/" not in l)]

    # L1: the calib behind the concat, shared by two convs
    def direct(p, n_in=2, axis=1):
        c = _cat(p, n_in, axis)
        _conv(p, "cat", "out", c, 4)
        _conv(p, "cat", "out2", c, 4)
    assert cats(_mini(lite, direct, ("out", "out2"))) == ["concat/int8 in=a,b out=cat +calib=cat/precision_trans scale=%s -f32 axis=1" % S05]
    # any number of inputs, any axis
    assert cats(_mini(lite, lambda p: direct(p, 3, 2), ("out", "out2"))) == ["concat/int8 in=a,b,c out=cat +calib=cat/precision_trans scale=%s -f32 axis=2" % S05]
    assert cats(_mini(lite, lambda p: direct(p, 3, -4), ("out", "out2"))) == ["concat/int8 in=a,b,c out=cat +calib=cat/precision_trans scale=%s -f32 axis=-4" % S05]
    # a fetched concat keeps its fp32 tensor
    assert cats(_mini(lite, direct, ("out", "out2", "cat"))) == ["concat/int8 in=a,b out=cat +calib=cat/precision_trans scale=%s axis=1" % S05]
    # the builder's default (on: DESIGN.md 12), the switch off, set_fuse(false)
    assert _mini(lite, direct, ("out", "out2"), fuse_concat=None) == _mini(lite, direct, ("out", "out2"))
    sep = ["concat/def in=a,b out=cat axis=1", "calib/fp32_to_int8 in=cat out=cat/precision_trans scale=%s" % S05]
    assert cats(_mini(lite, direct, ("out", "out2"), fuse_concat=False)) == sep
    assert cats(_mini(lite, direct, ("out", "out2"), fuse=False)) == sep

    # L2 alone: a max pool between the concat and the calib
    def pooled(p, kind="max", global_pooling=False, extra=None):
        c = _cat(p)
        _pool(p, "cat", "pl", kind, global_pooling)
        _conv(p, "pl", "out", c, 4)
        if extra:
            extra(p)
    assert cats(_mini(lite, pooled)) == ["concat/int8 in=a,b out=cat +calib=cat/precision_trans scale=%s -f32 axis=1" % S05,
                                         "pool2d/def in=cat/precision_trans out=pl/precision_trans int8"]
    untouched = ["concat/def in=a,b out=cat axis=1", "pool2d/def in=cat out=pl", "calib/fp32_to_int8 in=pl out=pl/precision_trans scale=%s" % S05]
    assert cats(_mini(lite, lambda p: pooled(p, "avg"))) == untouched                        # an average pool
    assert cats(_mini(lite, lambda p: pooled(p, "max", True))) == untouched                  # a global pool
    assert cats(_mini(lite, pooled, ("out", "pl"))) == untouched                             # a pool that is fetched
    two = _mini(lite, lambda p: pooled(p, extra=lambda q: q.graph_elementwise_add("pl", "pl", "twice")), ("out", "twice"))
    assert cats(two) == untouched                                                            # a pool with a second reader
    # a concat whose output only fp32 ops read
    assert cats(_mini(lite, lambda p: (_cat(p), p.graph_elementwise_add("cat", "cat", "out")))) == ["concat/def in=a,b out=cat axis=1"]

    # L1 and L2 together: one scale
    def both(p, pool_scale=0.05, kind="max"):
        c = _cat(p)
        _conv(p, "cat", "out", c, 4)
        _pool(p, "cat", "pl", kind)
        _conv(p, "pl", "out2", c, 4, pool_scale)
    assert cats(_mini(lite, both, ("out", "out2"))) == ["concat/int8 in=a,b out=cat +calib=cat/precision_trans scale=%s -f32 axis=1" % S05,
                                                        "pool2d/def in=cat/precision_trans out=pl/precision_trans int8"]
    # a pool whose calib scale differs from the direct calib's stays an fp32 reader, and so does an average pool beside the calib
    assert cats(_mini(lite, lambda p: both(p, 0.07), ("out", "out2"))) == [
        "concat/int8 in=a,b out=cat +calib=cat/precision_trans scale=%s axis=1" % S05, "pool2d/def in=cat out=pl",
        "calib/fp32_to_int8 in=pl out=pl/precision_trans scale=%s" % S07]
    assert cats(_mini(lite, lambda p: both(p, 0.05, "avg"), ("out", "out2"))) == [
        "concat/int8 in=a,b out=cat +calib=cat/precision_trans scale=%s axis=1" % S05, "pool2d/def in=cat out=pl",
        "calib/fp32_to_int8 in=pl out=pl/precision_trans scale=%s" % S05]

    # no direct calib and two pools of two scales: no one scale for the int8 copy
    def two_pools(p, s2):
        c = _cat(p)
        _pool(p, "cat", "pl", "max")
        _pool(p, "cat", "pm", "max")
        _conv(p, "pl", "out", c, 4, 0.05)
        _conv(p, "pm", "out2", c, 4, s2)
    assert cats(_mini(lite, lambda p: two_pools(p, 0.07), ("out", "out2"))) == [
        "concat/def in=a,b out=cat axis=1", "pool2d/def in=cat out=pl", "pool2d/def in=cat out=pm",
        "calib/fp32_to_int8 in=pl out=pl/precision_trans scale=%s" % S05, "calib/fp32_to_int8 in=pm out=pm/precision_trans scale=%s" % S07]
    assert cats(_mini(lite, lambda p: two_pools(p, 0.05), ("out", "out2"))) == [
        "concat/int8 in=a,b out=cat +calib=cat/precision_trans scale=%s -f32 axis=1" % S05,
        "pool2d/def in=cat/precision_trans out=pl/precision_trans int8", "pool2d/def in=cat/precision_trans out=pm/precision_trans int8"]

    # a concat K takes
    def shuffled(p):
        c = _cat(p)
        p.graph_shuffle_channel("cat", "shuf", 2)
        _conv(p, "shuf", "out", c, 4)
    assert cats(_mini(lite, shuffled)) == ["shuffle_channel/int8 in=a,b out=shuf +calib=shuf/precision_trans scale=%s -f32 via=cat" % S05]


# ------------------------------------------------------------------ ISA
def test_new_kernel_instances_use_no_scratch():
    """The ISA the build keeps beside shuffle_ops.o: three instances of concat_calib_kernel (16 floats, a quad, an element per
    lane), none with a private segment."""
    files = glob.glob(os.path.join(LITE, "csrc", "shuffle_ops-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert len(files) == 1, "build the library first (the ISA is kept beside the object)"
    text = open(files[0]).read()
    meta = re.findall(r"\.name:\s+(\S*concat_calib_kernel\S*)\n(?:(?!\s+\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(meta) == 3 and len({m[0] for m in meta}) == 3, meta
    assert all(size == "0" for _, size in meta), meta
    desc = re.findall(r"\.amdhsa_kernel (\S*concat_calib_kernel\S*)\n\s*(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size (\d+)", text)
    assert len(desc) == 3 and all(size == "0" for _, size in desc), desc
