"""CPU tests of the ShuffleNetV2 ops: the numpy restatements of concat / split / shuffle_channel (shuffle_oracle.py) against
independent formulations, the exported symbols and registered kernels, the param structs against the reference's, the lowering
of ShuffleNetV2 (unfused: the reference's instruction list; fused with K: one shuffle_channel/unit or shuffle_channel/int8 per
unit tail), the graphs K must leave alone, the malformed graphs the builder refuses, and the health of the synthetic network."""
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


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _special(rng, shape):
    x = (rng.standard_normal(shape) * 4).astype(F32)
    edge = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38], F32)
    k = min(x.size, edge.size)
    x.reshape(-1)[:k] = edge[:k]
    return x


# ------------------------------------------------------------------ helpers against independent formulations
@pytest.mark.parametrize("outer,cs,inner", [(1, [1, 1], 1), (3, [2, 5], 49), (2, [58, 58], 196), (2, [24, 24, 24], 16), (2, [3, 1, 4, 2], 7),
                                            (1, [1] * 9, 5), (6, [2, 3], 1)])
def test_concat_and_split_restatements(outer, cs, inner):
    rng = np.random.default_rng(sum(cs) + inner)
    xs = [_special(rng, (outer, c, inner)) for c in cs]
    y = S.concat(xs, 1)
    assert np.array_equal(_bits(y), _bits(np.concatenate(xs, axis=1)))
    parts = S.split(y, 1, sections=cs)
    want = np.split(y, np.cumsum(cs)[:-1], axis=1)
    assert len(parts) == len(cs)
    for p, w, x in zip(parts, want, xs):
        assert np.array_equal(_bits(p), _bits(w)) and np.array_equal(_bits(p), _bits(x))
    if len(set(cs)) == 1:
        for p, x in zip(S.split(y, 1, num=len(cs)), xs):
            assert np.array_equal(_bits(p), _bits(x))
    # other axes: 0 (outer = 1) and the last one (inner = 1), negative axis
    z = [x.reshape(c, outer, inner) for x, c in zip(xs, cs)]
    assert np.array_equal(_bits(S.concat(z, 0)), _bits(np.concatenate(z, axis=0)))
    t = [x.reshape(outer, inner, c) for x, c in zip(xs, cs)]
    assert np.array_equal(_bits(S.concat(t, -1)), _bits(np.concatenate(t, axis=2)))
    for p, w in zip(S.split(S.concat(t, 2), -1, sections=cs), t):
        assert np.array_equal(_bits(p), _bits(w))


@pytest.mark.parametrize("group", [2, 3, 4, 8])
def test_shuffle_channel_restatement_against_reshape_transpose_reshape(group):
    """shuffle_channel_fuse_pass.cc fuses exactly reshape [n, g, c/g, h, w] -> transpose(1, 2) -> reshape into the op."""
    import torch
    rng = np.random.default_rng(group)
    n, c, h, w = 3, 24, 5, 7
    x = _special(rng, (n, c, h, w))
    got = S.shuffle_channel(x, group)
    want = torch.from_numpy(x).reshape(n, group, c // group, h, w).transpose(1, 2).reshape(n, c, h, w).contiguous().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    # group 2 over a concat of two operands: shuffled channel c' is operand c' % 2, channel c' / 2
    a, b = x[:, :12], x[:, 12:]
    s = S.shuffle_channel(S.concat([a, b], 1), 2)
    assert np.array_equal(_bits(s[:, 0::2]), _bits(a)) and np.array_equal(_bits(s[:, 1::2]), _bits(b))
    lo, hi, q = S.shuffle_unit(a, b, 12, 0.05)
    assert np.array_equal(_bits(lo), _bits(s[:, :12])) and np.array_equal(_bits(hi), _bits(s[:, 12:]))
    assert np.array_equal(q, S.calib_i8(s[:, 12:], 0.05))
    lo, hi, _ = S.shuffle_unit(a, b, 0)
    assert lo.shape[1] == 0 and np.array_equal(_bits(hi), _bits(s))
    lo, hi, _ = S.shuffle_unit(a, b, 7)
    assert np.array_equal(_bits(lo), _bits(s[:, :7])) and np.array_equal(_bits(hi), _bits(s[:, 7:]))


def test_calib_restatement_equals_plref(plref):
    v = (np.random.default_rng(5).standard_normal(50000) * 3).astype(F32)
    v[:8] = [0.5, -0.5, 1.5, 2.5, -2.5, 126.5, 127.5, -1000]
    for s in (1.0, 0.05, 4.0 / 127):
        assert np.array_equal(S.calib_i8(v, s), plref.calib_f32_to_i8(v, s))


# ------------------------------------------------------------------ exports, registrations, structs
def test_new_symbols_are_exported_and_kernels_registered(pkg, lite):
    capi = pkg.capi
    L = capi.load()
    for name in ("plhip_concat_f32", "plhip_split_f32", "plhip_shuffle_channel_f32", "plhip_shuffle_unit_f32"):
        assert name in capi.EXPORTS and hasattr(L, name)
    # the route table's answer the graph builder asks before a conv takes its tail over: no for the direct 3x3 stride-2 stem
    assert "plhip_conv2d_fused_supported" in capi.EXPORTS
    import ctypes as C
    stem = capi.conv_desc(2, 3, 224, 224, 24, 3, 3, (1, 1, 1, 1), (2, 2), (1, 1), 1, act=capi.ACT_RELU)
    assert L.plhip_conv2d_fused_supported(C.byref(stem)) == 0
    for d in (capi.conv_desc(2, 64, 14, 14, 96, 1, 1), capi.conv_desc(2, 3, 224, 224, 64, 7, 7, (3, 3, 3, 3), (2, 2), (1, 1), 1),
              capi.conv_desc(2, 64, 28, 28, 64, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 1)):
        assert L.plhip_conv2d_fused_supported(C.byref(d)) == 1
    LL = lite.load()
    for name in ("pllite_graph_concat", "pllite_graph_split", "pllite_graph_shuffle_channel", "pllite_graph_set_fuse_shuffle"):
        assert hasattr(LL, name), name
    # concat/def, split/def, shuffle_channel/def + the two fusion products shuffle_channel/int8 and shuffle_channel/unit
    assert LL.pllite_registered_kernels(b"concat", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1
    assert LL.pllite_registered_kernels(b"split", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1
    assert LL.pllite_registered_kernels(b"shuffle_channel", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 3
    for op in (b"concat", b"split", b"shuffle_channel"):
        assert LL.pllite_registered_kernels(op, lite.PREC_INT8, lite.LAYOUT_NCHW) == 0, op
    src = open(os.path.join(LITE, "lite", "kernels", "hip", "shuffle_compute.cc")).read()
    regs = re.findall(r"REGISTER_LITE_KERNEL\((\w+), kHIP, kFloat, kNCHW, [\w:]+, (\w+)\)", src)
    assert sorted(regs) == sorted([("concat", "def"), ("split", "def"), ("shuffle_channel", "def"), ("shuffle_channel", "int8"),
                                   ("shuffle_channel", "unit")])


@pytest.mark.skipif(not os.path.isdir("/root/reference/lite"), reason="reference tree not present on this machine")
def test_shuffle_compute_compiles_against_the_reference_param_structs():
    """The method of test_boundary_reference_params.py: the generated header holds the reference's own struct text."""
    with tempfile.TemporaryDirectory(prefix="khip_refparams.") as tmp:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_ref_params_header.py"), "--out", tmp], stdout=subprocess.DEVNULL)
        gen = open(os.path.join(tmp, "lite", "operators", "op_params.h")).read()
        for name in ("struct ConcatParam", "struct SplitParam", "struct ShuffleChannelParam"):
            assert name in gen, name
        assert "hi_output" not in gen and "calib_output" not in gen
        p = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", tmp, "-I", LITE, "-I", os.path.join(ROOT, "include"),
                            os.path.join(LITE, "lite", "kernels", "hip", "shuffle_compute.cc")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "shuffle_compute.cc does not compile against the reference's structs:\n%s" % p.stdout.decode()[-3000:]


def test_new_param_structs_are_field_subsets_of_the_reference():
    if not os.path.isdir("/root/reference/lite"):
        pytest.skip("reference tree not present on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_ref_params_header as g
    assert {"ConcatParam", "SplitParam", "ShuffleChannelParam"} <= set(g.STRUCTS)
    ref = open("/root/reference/lite/operators/op_params.h").read()
    ours = open(os.path.join(LITE, "lite", "operators", "op_params.h")).read()
    for name, n_fields in (("ConcatParam", 4), ("SplitParam", 7), ("ShuffleChannelParam", 3)):
        mine, theirs = g.struct_text(ours, name), g.struct_text(ref, name)
        decls = re.findall(r"^\s+((?:const\s+)?[\w:<>\s\*]+?[\s\*&]\w+\s*(?:\{[^}]*\})?);", mine, re.M)
        assert len(decls) == n_fields, (name, decls)
        theirs_flat = re.sub(r"\s+", " ", theirs)
        for d in decls:  # the whole declaration (type, name, default) occurs in the reference's struct
            assert re.sub(r"\s+", " ", d) in theirs_flat, "%s: `%s` is not a field of the reference's struct" % (name, d)


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


def test_shufflenet_v2_structure(wl):
    for scale, widths in wl.SHUFFLENET_V2_WIDTHS.items():
        net = wl.shufflenet_v2_net(scale, res=64)
        ops = net["ops"]
        assert sum(o["op"] == "concat" for o in ops) == 16 == sum(o["op"] == "shuffle_channel" for o in ops)
        assert sum(o["op"] == "split" for o in ops) == 13
        assert [net["shapes"]["s%du1_shuffle" % (i + 2)][0] for i in range(3)] == list(widths)
        assert net["shapes"]["conv5"][0] == (2048 if scale == 2.0 else 1024) and net["shapes"]["prob"] == (1000, 1, 1)
        assert net["shapes"]["conv1"] == (24, 32, 32) and net["shapes"]["pool1"] == (24, 16, 16)
    net = wl.shufflenet_v2_net(1.0)
    assert net["shapes"]["s4u4_shuffle"] == (464, 7, 7) and net["shapes"]["s2u2_x2"] == (58, 28, 28)
    assert wl.shuffle_unit_bytes(net, 1) == (53 * (3 * 58 * 784 + 7 * 116 * 196 + 3 * 232 * 49), 13 * (3 * 58 * 784 + 7 * 116 * 196 + 3 * 232 * 49))


def test_shufflenet_v2_lowering(lite, wl):
    net = wl.shufflenet_v2_net(1.0)
    # ---- unfused: the reference's instruction list, restated independently by the helper oracle's plan()
    plan = _plan(lite, wl, net, fuse=False)
    heads = _heads(plan)
    assert heads.count("concat/def") == 16 and heads.count("shuffle_channel/def") == 16 and heads.count("split/def") == 13
    want = S.plan(net)
    body = plan[1:-1]
    assert len(body) == len(want)
    for line, (kind, s) in zip(body, want):
        head = line.split(" ")[0]
        if kind == "calib":
            assert head == "calib/fp32_to_int8" and ("out=" + s["dst"]) in line.split(" "), line
            continue
        o = s["o"]
        if o["op"] in S.INT8_OPS:
            alias = ("int8out" if s["int8_out"] else "fp32out") if o["op"] == "fc" else ("int8_out" if s["int8_out"] else "fp32_out")
        else:
            alias = "def"
        assert head == o["op"] + "/" + alias, line
        assert ("in=" + ",".join(s["ins"])) in line.split(" ") and ("out=" + ",".join(S.outs_of(o))) in line.split(" "), line
    # the precision rules: the last 1x1 conv of a branch writes fp32, the conv behind a split reads a calib of the second half
    for l in body:
        name = l.split("out=")[1].split(" ")[0]
        if name.endswith(("_r_pw2", "_l_pw")):
            assert l.startswith("conv2d/fp32_out"), l
        if name.endswith("_r_pw1") and not name.endswith("u1_r_pw1"):
            assert ("in=" + name[:-len("_r_pw1")] + "_x2/precision_trans") in l.split(" "), l
    # ---- with K: no concat / split / shuffle_channel line of its own, 13 unit and 3 int8 lines, 45 instructions fewer
    off = _plan(lite, wl, net, fuse=True, fuse_shuffle=False)
    on = _plan(lite, wl, net, fuse=True, fuse_shuffle=True)
    assert _plan(lite, wl, net, fuse=True) == on  # the builder's default: K on (measured)
    assert _heads(off).count("concat/def") == 16 and not [h for h in _heads(off) if h in ("shuffle_channel/unit", "shuffle_channel/int8")]
    h_on = _heads(on)
    assert not [h for h in h_on if h in ("concat/def", "split/def", "shuffle_channel/def")]
    assert h_on.count("shuffle_channel/unit") == 13 and h_on.count("shuffle_channel/int8") == 3
    assert len(off) - len(on) == 45 == 13 * 3 + 3 * 2
    units = [l for l in on if l.startswith("shuffle_channel/unit")]
    for l in units:  # in = the concat's operands, out = the first half, the second half int8 only, three names no longer written
        kv = dict(f.split("=", 1) for f in l.split(" ")[1:] if "=" in f)
        blk = kv["out"][:-len("_x1")]
        assert kv["out"] == blk + "_x1" and kv["+calib"] == blk + "_x2/precision_trans" and "+hi" not in kv, l
        assert kv["via"].split(",")[2] == blk + "_x2" and kv["via"].split(",")[0].endswith("_concat") and len(kv["in"].split(",")) == 2, l
        assert float(kv["scale"]) > 0
    for l in [l for l in on if l.startswith("shuffle_channel/int8")]:
        kv = dict(f.split("=", 1) for f in l.split(" ")[1:] if "=" in f)
        assert kv["+calib"] == kv["out"] + "/precision_trans" and l.split(" ")[-2] == "-f32" and kv["via"].endswith("_concat"), l
    assert {l.split("out=")[1].split(" ")[0] for l in on if l.startswith("shuffle_channel/int8")} == {"s2u4_shuffle", "s3u8_shuffle", "s4u4_shuffle"}
    # the other fusions fire as before: every line that is not one of K's is a line of the K-off plan, in its order
    rest_on = [l for l in on if not l.startswith("shuffle_channel/")]
    rest_off = [l for l in off if not l.startswith(("concat/", "split/", "shuffle_channel/")) and
                not (l.startswith("calib/") and l.split("in=")[1].split(" ")[0].endswith(("_x2", "_shuffle")))]
    assert rest_on == rest_off
    # the direct 3x3 stride-2 stem has no fused tail: stem, max pool and calib stay three instructions
    # (what it does take over is the calib in front of it, fusion F, as the MobileNet stems do)
    assert any(l.startswith("conv2d/fp32_out in=image/target_trans out=conv1 +calib_in=image/precision_trans") and "+calib=" not in l for l in on)
    assert "pool2d/def in=conv1 out=pool1" in on
    assert any(l.startswith("calib/fp32_to_int8 in=pool1 out=pool1/precision_trans") for l in on)
    # K needs set_fuse(true)
    assert _plan(lite, wl, net, fuse=False, fuse_shuffle=True) == plan
    # program_costs follows every plan; the unit lines carry the 13 h P of the issue's table
    for pl in (plan, off, on):
        costs = wl.program_costs(net, 2, pl)
        assert len(costs) == len(pl) and all(c["bytes"] >= 0 for c in costs)
    costs = wl.program_costs(net, 2, on)
    assert sum(c["bytes"] for c in costs if c["family"] == "shuffle_unit") == wl.shuffle_unit_bytes(net, 2)[1]
    sep = wl.program_costs(net, 2, plan)
    moved = sum(c["bytes"] for c, l in zip(sep, plan) if l.startswith(("split/", "shuffle_channel/")) or
                (l.startswith("concat/") and not l.split("out=")[1].startswith(("s2u4", "s3u8", "s4u4"))) or
                (l.startswith("calib/") and l.split("in=")[1].split(" ")[0].endswith("_x2")))
    # 53 h P per stride-1 unit; the three shuffle_channel lines in front of a stride-2 unit / the head are not part of a unit tail
    extra = sum(c["bytes"] for c, l in zip(sep, plan) if l.startswith("shuffle_channel/") and l.split("out=")[1].startswith(("s2u4", "s3u8", "s4u4")))
    assert moved - extra == wl.shuffle_unit_bytes(net, 2)[0]


def _mini(lite, build, fuse_shuffle=True, fetch=("out",)):
    """A planner graph: feed x [2, 8, 4, 4] -> two 1x1 convs a, b (fp32 out) -> build(p) -> int8 conv(s) reading the result."""
    p = lite.Predictor(planner=True)
    try:
        p.graph_set_fuse(True)
        p.graph_set_fuse_shuffle(fuse_shuffle)
        p.graph_feed("x", (2, 8, 4, 4))
        build(p)
        for f in fetch:
            p.graph_fetch(f)
        return p.graph_plan()
    finally:
        p.close()


def _conv(p, src, dst, cin, cout):
    w = np.ones((cout, cin, 1, 1), np.int8)
    p.graph_conv("conv2d", src, dst, w, None, (1, 1), (0, 0, 0, 0), (1, 1), 1, 1, 0.0, 0.05, np.full(cout, 0.01, F32))


def _unit_graph(p, n_in=2, cb=8, group=2, num=2, sections=(), extra=None):
    _conv(p, "x", "a", 8, 8)
    _conv(p, "x", "b", 8, cb)
    srcs = ["a", "b"] + (["a2"] if n_in == 3 else [])
    if n_in == 3:
        _conv(p, "x", "a2", 8, 8)
    p.graph_concat(srcs, "cat", 1)
    p.graph_shuffle_channel("cat", "shuf", group)
    p.graph_split("shuf", ["lo", "hi"], 1, num, sections)
    _conv(p, "hi", "out", (8 + cb + (8 if n_in == 3 else 0)) // 2 if num else sections[1], 4)
    if extra:
        extra(p)


def test_fusion_k_fires_only_on_its_pattern(lite):
    fused = _mini(lite, _unit_graph)
    assert _heads(fused).count("shuffle_channel/unit") == 1 and not [h for h in _heads(fused) if h in ("concat/def", "split/def", "shuffle_channel/def")]
    assert _heads(fused).count("calib/fp32_to_int8") == 1  # the one in front of the two convs that read the feed
    line = [l for l in fused if l.startswith("shuffle_channel/unit")][0]
    assert line == "shuffle_channel/unit in=a,b out=lo +calib=hi/precision_trans scale=0.0500000007 via=cat,shuf,hi", line
    # equal sections written out are the same split
    assert _heads(_mini(lite, lambda p: _unit_graph(p, num=0, sections=(8, 8)))).count("shuffle_channel/unit") == 1
    # the fp32 second half is written where it has another reader (here: a fetch)
    both = _mini(lite, _unit_graph, fetch=("out", "hi"))
    assert [l for l in both if l.startswith("shuffle_channel/unit")][0] == \
        "shuffle_channel/unit in=a,b out=lo +hi=hi +calib=hi/precision_trans scale=0.0500000007 via=cat,shuf"
    # with the switch off
    assert "concat/def" in _heads(_mini(lite, _unit_graph, fuse_shuffle=False))

    def separate(plan):
        h = _heads(plan)
        return "concat/def" in h and "shuffle_channel/def" in h and not [x for x in h if x in ("shuffle_channel/unit", "shuffle_channel/int8")]
    assert separate(_mini(lite, lambda p: _unit_graph(p, n_in=3)))                       # three inputs
    assert separate(_mini(lite, lambda p: _unit_graph(p, cb=24, group=2, num=2)))        # unequal channels
    assert separate(_mini(lite, lambda p: _unit_graph(p, group=4)))                      # another group
    assert separate(_mini(lite, lambda p: _unit_graph(p, num=0, sections=(4, 12))))      # unequal sections
    assert separate(_mini(lite, _unit_graph, fetch=("out", "cat")))                      # an intermediate that is fetched
    assert separate(_mini(lite, _unit_graph, fetch=("out", "shuf")))
    assert separate(_mini(lite, lambda p: _unit_graph(p, extra=lambda q: q.graph_elementwise_add("cat", "cat", "twice")), fetch=("out", "twice")))

    # K2: the shuffled tensor read by int8 convs through one shared calib; the fp32 tensor stays where something else reads it
    def k2(p, n_in=2):
        _conv(p, "x", "a", 8, 8)
        _conv(p, "x", "b", 8, 8)
        if n_in == 3:
            _conv(p, "x", "c", 8, 8)
        p.graph_concat(["a", "b"] + (["c"] if n_in == 3 else []), "cat", 1)
        p.graph_shuffle_channel("cat", "shuf", 2)
        _conv(p, "shuf", "out", 8 * n_in, 4)
        _conv(p, "shuf", "out2", 8 * n_in, 4)
    pl = _mini(lite, k2, fetch=("out", "out2"))
    assert [l for l in pl if l.startswith("shuffle_channel/")] == \
        ["shuffle_channel/int8 in=a,b out=shuf +calib=shuf/precision_trans scale=0.0500000007 -f32 via=cat"]
    pl = _mini(lite, k2, fetch=("out", "out2", "shuf"))
    assert [l for l in pl if l.startswith("shuffle_channel/")] == \
        ["shuffle_channel/int8 in=a,b out=shuf +calib=shuf/precision_trans scale=0.0500000007 via=cat"]
    assert separate(_mini(lite, lambda p: k2(p, 3), fetch=("out", "out2")))


def test_malformed_graphs_are_refused_by_the_builder(lite):
    def plan(build):
        p = lite.Predictor(planner=True)
        try:
            p.graph_feed("x", (2, 8, 4, 4))
            p.graph_feed("y", (2, 8, 4, 5))
            build(p)
            return p.graph_plan()
        finally:
            p.close()
    with pytest.raises(lite.LiteError, match=r"concat c: input y \{2,8,4,5\} differs from x \{2,8,4,4\} outside axis 1"):
        plan(lambda p: p.graph_concat(["x", "y"], "c", 1))
    plan(lambda p: p.graph_concat(["x", "y"], "c", 3))  # the same operands along the axis in which they differ
    with pytest.raises(lite.LiteError, match=r"split x: num 3 does not divide the axis \(8\)"):
        plan(lambda p: p.graph_split("x", ["a", "b", "c"], 1, 3))
    with pytest.raises(lite.LiteError, match=r"split x: the sections do not add up to the axis \(7 of 8\)"):
        plan(lambda p: p.graph_split("x", ["a", "b"], 1, 0, (3, 4)))
    with pytest.raises(lite.LiteError, match=r"split x: 3 sections but 2 outputs"):
        plan(lambda p: p.graph_split("x", ["a", "b"], 1, 0, (3, 4, 1)))
    with pytest.raises(lite.LiteError, match=r"shuffle_channel s: group 3 does not divide C = 8"):
        plan(lambda p: p.graph_shuffle_channel("x", "s", 3))
    with pytest.raises(lite.LiteError, match=r"variable b is written twice"):
        plan(lambda p: (p.graph_split("x", ["a", "b"], 1, 2), p.graph_shuffle_channel("a", "b", 2)))
    with pytest.raises(lite.LiteError, match=r"variable a is written twice"):
        plan(lambda p: p.graph_split("x", ["a", "a"], 1, 2))
    with pytest.raises(lite.LiteError, match=r"input nowhere is not produced"):
        plan(lambda p: p.graph_concat(["x", "nowhere"], "c", 1))
    # every output of a split is a variable with consumers of its own
    ok = plan(lambda p: (p.graph_split("x", ["a", "b"], 1, 0, (3, 5)), p.graph_concat(["b", "a"], "c", 1), p.graph_fetch("c")))
    assert "split/def in=x/target_trans out=a,b axis=1 sections=3,5" in ok and "concat/def in=b,a out=c axis=1" in ok


# ------------------------------------------------------------------ generator health, on the oracle alone
def _shares(ref):
    """name -> (share of values at +-127, share of zeros, channels) of every int8 activation tensor."""
    return {k: ((np.abs(v.astype(np.int32)) == 127).mean(), (v == 0).mean(), v.shape[1]) for k, v in ref.items() if v.dtype == np.int8}


def test_synthetic_network_is_as_healthy_as_mobilenet_v2(wl, plref):
    """The yardstick is computed here, not written down: the worst int8 tensor of mobilenet_v2_net on the same images (saturated
    share 0.048, zero share 0.637 when this was written).  Every int8 activation tensor of both ShuffleNets is at or below it in
    both shares (measured worst: saturated 0.042 at 1.0 and 0.046 at 0.5; zeros 0.603 at 1.0 and 0.613 at 0.5)."""
    import oracle.graph_oracle as GO
    img = np.random.default_rng(350).uniform(-1, 1, (2, 3, 224, 224)).astype(F32)
    mb = _shares(GO.forward(plref, wl.mobilenet_v2_net(), img, via_gemm=True))
    worst_sat, worst_zero = max(v[0] for v in mb.values()), max(v[1] for v in mb.values())
    assert 0 < worst_sat < 0.1 and 0.5 < worst_zero < 0.8
    for scale in (1.0, 0.5):
        net = wl.shufflenet_v2_net(scale)
        ref = S.forward(plref, net, img, via_gemm=True)
        sh = _shares(ref)
        assert len(sh) > 50
        print("scale %.1f: worst saturated %.4f (yardstick %.4f), worst zero %.4f (yardstick %.4f)" % (
            scale, max(v[0] for v in sh.values()), worst_sat, max(v[1] for v in sh.values()), worst_zero))
        for name, (sat, zero, c) in sh.items():
            assert sat <= worst_sat, (scale, name, sat, worst_sat)
            assert zero <= worst_zero, (scale, name, zero, worst_zero)
        # the calibs of the concatenated tensors (one scale for both operands) are among them
        assert len([k for k in sh if k.endswith(("_x2/precision_trans", "_shuffle/precision_trans"))]) == 16
        assert ref["prob"].shape == (2, 1000) and np.isfinite(ref["prob"]).all()
