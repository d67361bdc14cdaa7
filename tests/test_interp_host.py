"""CPU tests of the dense-prediction ops: interp_oracle against torch.nn.functional.interpolate and against a float64 evaluation of
the stated formulas; arg_max's tie rule, output types and keepdims; the exported symbols; the kept ISA of csrc/interp_ops.hip (no
private segment, no fused multiply-add in any of its kernels, LDS only in the fused kernel)."""
import glob
import os
import re

import numpy as np
import pytest

import interp_oracle as I

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITE = os.path.join(ROOT, "paddle-lite_amd")
# (planes, in_h, in_w, out_h, out_w): test_gpu_interp.py's cases
CASES = [(1, 1, 1, 1, 1), (3, 1, 1, 4, 5), (2, 2, 2, 2, 2), (6, 7, 5, 28, 20), (4, 8, 8, 15, 17), (2, 16, 16, 64, 64),
         (3, 9, 13, 4, 6), (1, 3, 3, 1, 7), (2, 33, 33, 129, 129)]


def _close(got, want, x):
    """The project's fp32 rule: rtol 1e-5 plus atol 1e-5 * max|x|.  The two orders of operations differ by at most 6 roundings of a
    value bounded by the largest corner."""
    return np.allclose(got, want, rtol=1e-5, atol=1e-5 * float(np.abs(x).max()))


# ------------------------------------------------------------------ the oracle
def test_oracle_equals_torch_interpolate():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(570)
    for planes, ih, iw, oh, ow in CASES:
        x = (rng.standard_normal((1, planes, ih, iw)) * 2).astype(F32)
        t = torch.from_numpy(x)
        for method, ac, am, kw in (("bilinear", True, 1, dict(mode="bilinear", align_corners=True)),
                                   ("bilinear", False, 0, dict(mode="bilinear", align_corners=False)),
                                   ("nearest", False, 1, dict(mode="nearest"))):
            want = torch.nn.functional.interpolate(t, size=(oh, ow), **kw).numpy()
            got = I.interp(x, (oh, ow), method, ac, am)
            assert got.shape == want.shape and got.dtype == F32
            assert _close(got, want, x), ((planes, ih, iw, oh, ow), method, ac, float(np.abs(got - want).max()))


def _axis64(n_in, n_out, align_corners, nearest):
    """One axis of the stated rule, a scalar loop: the ratio and the coordinate are the fp32 values the rule names (they pick the
    source pixels), the weights are taken from them in float64."""
    r = I.ratio(n_in, n_out, align_corners)
    taps = []
    for l in range(n_out):
        f = F32(r * F32(l))
        if nearest:
            i = min(int(float(f) + 0.5), n_in - 1)
            taps.append((i, i, 1.0, 0.0))
        else:
            i0 = min(int(f), n_in - 1)
            w1 = float(f) - i0
            taps.append((i0, min(i0 + 1, n_in - 1), 1.0 - w1, w1))
    return taps


def test_oracle_equals_a_float64_evaluation_of_mode_1_and_of_aligned_nearest():
    rng = np.random.default_rng(571)
    for planes, ih, iw, oh, ow in CASES:
        if (ih, iw) == (oh, ow):
            continue
        x = (rng.standard_normal((planes, ih, iw)) * 2).astype(F32)
        x64 = x.astype(np.float64)
        for method, ac in (("bilinear", False), ("nearest", True)):
            ty, tx = _axis64(ih, oh, ac, method == "nearest"), _axis64(iw, ow, ac, method == "nearest")
            want = np.empty((planes, oh, ow))
            for k, (y0, y1, b0, b1) in enumerate(ty):
                for l, (x0, x1, a0, a1) in enumerate(tx):
                    want[:, k, l] = (x64[:, y0, x0] * a0 + x64[:, y0, x1] * a1) * b0 + (x64[:, y1, x0] * a0 + x64[:, y1, x1] * a1) * b1
            got = I.interp(x, (oh, ow), method, ac, 1)
            if method == "nearest":
                assert np.array_equal(got, want.astype(F32)), (planes, ih, iw, oh, ow)
            else:
                assert _close(got, want, x), ((planes, ih, iw, oh, ow), float(np.abs(got - want).max()))


def test_oracle_corner_rules():
    x = np.arange(12, dtype=F32).reshape(1, 3, 4)
    x[0, 1, 1] = -0.0
    for method in ("bilinear", "nearest"):
        for ac in (False, True):
            for am in (0, 1):
                same = I.interp(x, (3, 4), method, ac, am)     # in == out on both axes: the bits
                assert same is not x and np.array_equal(same.view(np.uint32), x.view(np.uint32))
                one = I.interp(x, (1, 1), method, ac, am)      # out == 1: ratio 0 with aligned corners
                if ac or method == "nearest" or am == 1:
                    assert one.shape == (1, 1, 1) and one[0, 0, 0] == x[0, 0, 0]
                up = I.interp(x[:, :1, :1], (5, 2), method, ac, am)   # in == 1: every tap is the one pixel
                assert up.shape == (1, 5, 2) and (up == x[0, 0, 0]).all()
    # aligned nearest rounds half up in DOUBLE: in 4 -> out 7 steps by 0.5, indices 0 1 1 2 2 3 3
    assert I.nearest_index(4, 7, True).tolist() == [0, 1, 1, 2, 2, 3, 3]
    assert I.nearest_index(4, 8, False).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    # the source index is clamped to in - 1 (a ratio that rounded up could reach `in`)
    for n_in, n_out in ((3, 7), (33, 129), (7, 1000)):
        for ac in (False, True):
            assert I.nearest_index(n_in, n_out, ac).max() == n_in - 1
            for am in (0, 1):
                i0, i1, w0, w1 = I.bilinear_taps(n_in, n_out, ac, am)
                assert i0.min() >= 0 and i1.max() == n_in - 1 and (i1 - i0).max() <= 1 and (w1 >= 0).all() and (w1 <= 1).all()


def test_arg_max_ties_types_and_keepdims():
    x = np.array([[[1, 5, 2], [7, 5, 2], [7, 1, 2]], [[0, 0, 3], [0, 9, 3], [0, 9, -1]]], F32)   # [2, 3, 3]
    assert I.arg_max(x, 1).tolist() == [[2, 1, 2], [2, 2, 1]]      # the LARGEST index among equal maxima
    assert np.argmax(x, axis=1).tolist() == [[1, 0, 0], [0, 1, 0]]  # ... where numpy takes the first
    for dtype, np_t in ((-1, np.int64), (3, np.int64), (2, np.int32)):
        for axis in (0, 1, 2, -1):
            got = I.arg_max(x, axis, dtype)
            keep = I.arg_max(x, axis, dtype, keepdims=True)
            assert got.dtype == np_t and keep.dtype == np_t
            ax = axis % 3
            assert got.shape == x.shape[:ax] + x.shape[ax + 1:] and keep.shape == x.shape[:ax] + (1,) + x.shape[ax + 1:]
            assert np.array_equal(np.squeeze(keep, ax), got)
            assert np.array_equal(np.take_along_axis(x, keep.astype(np.int64), ax), x.max(axis=ax, keepdims=True))
    for bad in (0, 1, 4, 5, -2):
        with pytest.raises(ValueError):
            I.arg_max(x, 1, bad)


# ------------------------------------------------------------------ exports and the kept ISA
def test_new_symbols_are_exported(pkg):
    capi = pkg.capi
    L = capi.load()
    for name in ("plhip_interp_f32", "plhip_arg_max_f32", "plhip_interp_argmax_f32"):
        assert name in capi.EXPORTS and hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "plhip.h")).read()
    for name in ("plhip_interp_f32", "plhip_arg_max_f32", "plhip_interp_argmax_f32"):
        assert re.search(r"plhip_status %s\(plhip_ctx\* ctx" % name, text), name
    for helper in ("interp", "arg_max", "interp_argmax"):
        assert hasattr(capi.Context, helper), helper
    # refusals need no device: a NULL context is refused with the entry point's own text
    assert L.plhip_interp_f32(None, None, 1, 1, 1, 1, 1, 0, 0, 0, None, None, 1.0) < 0
    assert L.plhip_last_error(None).decode().startswith("plhip_interp_f32: ")
    assert L.plhip_arg_max_f32(None, None, 1, 1, 1, None, -1) < 0
    assert L.plhip_last_error(None).decode().startswith("plhip_arg_max_f32: ")
    assert L.plhip_interp_argmax_f32(None, None, 1, 1, 1, 1, 1, 1, 0, 0, 0, None, -1) < 0
    assert L.plhip_last_error(None).decode().startswith("plhip_interp_argmax_f32: ")


def _kernels(text):
    """name -> body of every kernel in a kept .s file."""
    out = {}
    for m in re.finditer(r"^(_ZN5plhip\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        out[m.group(1)] = m.group(2)
    return out


def test_kept_isa_has_no_scratch_and_no_contraction():
    """The ISA the build keeps beside interp_ops.o: two instances of interp_kernel (a quad, an element per lane), four of
    arg_max_kernel (x int32 / int64 labels), two of interp_argmax_kernel; none with a private segment; no fused or packed fp32
    arithmetic in any (every product and sum of the interpolation rounds on its own); LDS reads only in the fused kernel, and no
    flat access anywhere (the LDS walk and the global walk are separate code)."""
    files = glob.glob(os.path.join(LITE, "csrc", "interp_ops-hip-amdgcn-amd-amdhsa-gfx950.s"))
    assert len(files) == 1, "build the library first (the ISA is kept beside the object)"
    text = open(files[0]).read()
    meta = re.findall(r"\.name:\s+(_ZN5plhip\S+)\n(?:(?!\s+\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
    names = sorted(m[0] for m in meta)
    assert len(names) == 8 and len(set(names)) == 8, names
    assert sum("13interp_kernel" in n for n in names) == 2 and sum("14arg_max_kernel" in n for n in names) == 4
    assert sum("20interp_argmax_kernel" in n for n in names) == 2
    assert all(size == "0" for _, size in meta), meta
    bodies = _kernels(text)
    assert sorted(bodies) == names
    for name, body in bodies.items():
        ops = set(re.findall(r"^\s+([a-z]\w+)", body, re.M))
        fused = sorted(o for o in ops if re.match(r"v_(fma|fmac|mac|mad)_f|v_pk_\w+_f32|v_dot", o))
        assert not fused, (name, fused)
        assert not [o for o in ops if o.startswith(("scratch_", "flat_"))], name
        assert any(o.startswith("ds_read") for o in ops) == ("interp_argmax" in name), name
        if "interp" in name:
            assert "v_mul_f32_e32" in ops or "v_mul_f32_e64" in ops, name


# ------------------------------------------------------------------ the plugin layer: registration, structs
import importlib  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import tempfile  # noqa: E402

import shuffle_oracle as S  # noqa: E402


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


@pytest.fixture(scope="module")
def segnet(wl):
    return wl.seg_mini_net()


def test_plugin_symbols_are_exported_and_the_kernels_registered(lite):
    LL = lite.load()
    for name in ("pllite_add_interp", "pllite_add_arg_max", "pllite_add_interp_arg_max", "pllite_graph_interp", "pllite_graph_arg_max",
                 "pllite_graph_set_fuse_interp_argmax", "pllite_graph_set_fuse_interp_calib"):
        assert hasattr(LL, name), name
    for name in ("add_interp", "add_arg_max", "add_interp_arg_max", "graph_interp", "graph_arg_max", "graph_set_fuse_interp_argmax",
                 "graph_set_fuse_interp_calib"):
        assert hasattr(lite.Predictor, name), name
    # the int8 aliases read fp32 and write int8: registered at kAny, so that def stays the one kernel a pick at kFloat finds
    for op in (b"bilinear_interp", b"nearest_interp"):
        assert LL.pllite_registered_kernels(op, lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1
        assert LL.pllite_registered_kernels(op, lite.PREC_ANY, lite.LAYOUT_NCHW) == 1
    assert LL.pllite_registered_kernels(b"arg_max", lite.PREC_ANY, lite.LAYOUT_NCHW) == 2
    assert LL.pllite_registered_kernels(b"arg_max", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 0
    src = open(os.path.join(LITE, "lite", "kernels", "hip", "interp_compute.cc")).read()
    assert re.findall(r"REGISTER_LITE_KERNEL\((\w+), kHIP, (\w+), kNCHW, [\w:]+, (\w+)\)", src) == [
        ("bilinear_interp", "kFloat", "def"), ("nearest_interp", "kFloat", "def"), ("bilinear_interp", "kAny", "int8"),
        ("nearest_interp", "kAny", "int8"), ("arg_max", "kAny", "def"), ("arg_max", "kAny", "interp")]


@pytest.mark.skipif(not os.path.isdir("/root/reference/lite"), reason="reference tree not present on this machine")
def test_interp_compute_compiles_against_the_reference_param_structs():
    """The method of test_boundary_reference_params.py: the generated header holds the reference's own struct text, and the fusion
    state lives in the side header."""
    with tempfile.TemporaryDirectory(prefix="khip_refparams.") as tmp:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_ref_params_header.py"), "--out", tmp], stdout=subprocess.DEVNULL)
        gen = open(os.path.join(tmp, "lite", "operators", "op_params.h")).read()
        assert "struct InterpolateParam" in gen and "struct ArgmaxParam" in gen and "calib_output" not in gen
        side = open(os.path.join(LITE, "lite", "kernels", "hip", "calib_tail.h")).read()
        assert "calib_output" in side and "calib_scale" in side and "drop_fp32_output" in side
        assert "HipInterpArgmaxFusion" in open(os.path.join(LITE, "lite", "kernels", "hip", "interp_fusion.h")).read()
        p = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", tmp, "-I", LITE, "-I", os.path.join(ROOT, "include"),
                            os.path.join(LITE, "lite", "kernels", "hip", "interp_compute.cc")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "interp_compute.cc does not compile against the reference's structs:\n%s" % p.stdout.decode()[-3000:]


@pytest.mark.skipif(not os.path.isdir("/root/reference/lite"), reason="reference tree not present on this machine")
def test_interpolate_and_argmax_params_are_subsets_of_the_reference_fields():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_ref_params_header as g
    ref = open("/root/reference/lite/operators/op_params.h").read()
    ours = open(os.path.join(LITE, "lite", "operators", "op_params.h")).read()
    for name, n_fields in (("InterpolateParam", 12), ("ArgmaxParam", 5)):
        mine, theirs = g.struct_text(ours, name), g.struct_text(ref, name)
        fields = re.findall(r"^\s+(?:const\s+)?[\w:<>\s\*]+?[\s\*&](\w+)\s*(?:\{[^}]*\})?;", mine, re.M)
        assert len(fields) == n_fields, (name, fields)
        missing = [f for f in fields if not re.search(r"\b%s\b" % f, theirs)]
        assert not missing, "%s has fields the reference lacks: %s" % (name, missing)


# ------------------------------------------------------------------ InferShapes and the fatal cases
def _mini(lite, build, fetch=("out",), fuse=True, m=True, n=True):
    """A planner graph: feed x [2, 8, 4, 4] -> build(p) -> the fetches."""
    p = lite.Predictor(planner=True)
    try:
        p.graph_set_fuse(fuse)
        if m is not None:
            p.graph_set_fuse_interp_argmax(m)
        if n is not None:
            p.graph_set_fuse_interp_calib(n)
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


def test_infer_shapes_and_the_fatal_cases(lite):
    """concat CHECKs that its operands differ along the axis only, so a concat that plans proves the shapes InferShapes gave."""
    def sizes(p):
        p.graph_interp("bilinear_interp", "x", "a", (8, 12), 0.0, False, 1)      # [2, 8, 8, 12]
        p.graph_interp("nearest_interp", "a", "b", None, 0.5, True, 1)           # by scale: int(8 * 0.5) x int(12 * 0.5) = [2, 8, 4, 6]
        p.graph_interp("nearest_interp", "b", "c", (8, 12), 2.0, False, 0)       # out_h / out_w win over the scale
        p.graph_concat(["a", "c"], "cat", 1)                                     # [2, 16, 8, 12]
        p.graph_arg_max("cat", "lab", 1, 2, True)                                # [2, 1, 8, 12]
        p.graph_arg_max("cat", "lab3", 3, -1, False)                             # [2, 16, 8]
        p.graph_arg_max("lab3", "lab2", -1, 3, True)                             # [2, 16, 1]
        p.graph_concat(["lab", "a"], "out", 1)                                   # [2, 9, 8, 12]: the kept axis has extent 1
        p.graph_concat(["lab3", "lab2"], "out2", 2)                              # [2, 16, 9]
    plan = _mini(lite, sizes, fetch=("out", "out2"))
    assert "nearest_interp/def in=a out=b by=0.5 align_corners=1 align_mode=1" in plan
    assert "nearest_interp/def in=b out=c size=8x12 align_corners=0 align_mode=0" in plan
    assert "arg_max/def in=cat out=lab axis=1 dtype=2 keepdims=1" in plan

    def fatal(words, build):
        with pytest.raises(lite.LiteError) as e:
            _mini(lite, build)
        assert words in str(e.value), str(e.value)
    fatal("differs from", lambda p: (p.graph_interp("bilinear_interp", "x", "a", (8, 8)), p.graph_concat(["a", "x"], "out", 1)))
    fatal("differs from", lambda p: (p.graph_interp("bilinear_interp", "x", "a", (4, 4)), p.graph_arg_max("a", "l", 1), p.graph_concat(["l", "x"], "out", 1)))
    fatal("neither out_h / out_w nor a scale", lambda p: p.graph_interp("bilinear_interp", "x", "out", None, 0.0))
    fatal("neither out_h / out_w nor a scale", lambda p: p.graph_interp("nearest_interp", "x", "out", (8, -1), 0.0))
    fatal("is empty", lambda p: p.graph_interp("nearest_interp", "x", "out", None, 0.2))
    fatal("align_mode", lambda p: p.graph_interp("bilinear_interp", "x", "out", (8, 8), 0.0, False, 2))
    fatal("is not [N, C, H, W]", lambda p: (p.graph_arg_max("x", "l", 1), p.graph_interp("bilinear_interp", "l", "out", (8, 8))))
    fatal("outside the rank", lambda p: p.graph_arg_max("x", "out", 4))
    fatal("outside the rank", lambda p: p.graph_arg_max("x", "out", -5))
    for bad in (0, 1, 4):
        fatal("dtype", lambda p, bad=bad: p.graph_arg_max("x", "out", 1, bad))
    fatal("op type", lambda p: p.graph_interp("trilinear_interp", "x", "out", (8, 8)))


# ------------------------------------------------------------------ the lowering of seg_mini_net
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


def _rule_mn(plan, m, n):
    """Rules M and N restated over a plan that was made without them.  Returns (new plan, interps M took, interps N took)."""
    lines = list(plan)
    dead = set()

    def readers(v):
        return [j for j, l in enumerate(lines) if j not in dead and (v in _kv(l)["in"].split(",") or _kv(l).get("+add") == v)]

    took_m, took_n = [], []
    for i, line in enumerate(plan):
        head = line.split(" ")[0]
        if head not in ("bilinear_interp/def", "nearest_interp/def"):
            continue
        kv = _kv(line)
        out, r = kv["out"], readers(kv["out"])
        attrs = line.split(" out=" + out, 1)[1]    # " size=.. align_corners=.. align_mode=.."
        if m and len(r) == 1 and lines[r[0]].startswith("arg_max/def ") and _kv(lines[r[0]])["in"] == out and _kv(lines[r[0]])["axis"] in ("1", "-3"):
            a = _kv(lines[r[0]])
            lines[i] = "arg_max/interp in=%s out=%s +interp=%s%s axis=%s dtype=%s keepdims=%s via=%s" % (
                kv["in"], a["out"], head.split("/")[0], attrs, a["axis"], a["dtype"], a["keepdims"], out)
            dead.add(r[0])
            took_m.append(out)
            continue
        calibs = [j for j in r if lines[j].startswith("calib/fp32_to_int8 ")]
        if n and calibs:
            assert len(calibs) == 1
            c = _kv(lines[calibs[0]])
            dead.add(calibs[0])
            lines[i] = "%s/int8 in=%s out=%s%s +calib=%s scale=%s%s" % (head.split("/")[0], kv["in"], out, attrs, c["out"], c["scale"],
                                                                     "" if readers(out) else " -f32")
            took_n.append(out)
    return [l for j, l in enumerate(lines) if j not in dead], took_m, took_n


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
        alias = ("int8_out" if s["int8_out"] else "fp32_out") if o["op"] in S.INT8_OPS else "def"
        assert head == o["op"] + "/" + alias, line
        assert ("in=" + ",".join(s["ins"])) in toks and ("out=" + o["name"]) in toks, line


def test_structure_of_seg_mini_net(wl, segnet):
    ops, sh = segnet["ops"], segnet["shapes"]
    assert segnet["input_shape"] == (3, 64, 64) and segnet["output"] == "label" and sh["label"] == (64, 64)
    assert [o["op"] for o in ops if "interp" in o["op"] or o["op"] == "arg_max"] == ["bilinear_interp", "nearest_interp", "bilinear_interp", "arg_max"]
    assert sh["stem"] == (16, 32, 32) and sh["enc1_pw"] == (24, 16, 16) and sh["enc3_pw"] == (64, 8, 8)
    assert sh["aspp_concat"] == (96, 8, 8) and sh["aspp_project"] == (32, 8, 8) and sh["dec_up1"] == (32, 16, 16)
    assert sh["dec_concat"] == (48, 16, 16) and sh["dec_up2"] == (32, 32, 32) and sh["logits"] == (19, 32, 32) and sh["logits_up"] == (19, 64, 64)
    by = {o["name"]: o for o in ops}
    assert by["aspp_d2"]["dilation"] == 2 and by["aspp_d2"]["pad"] == 2 and by["aspp_d3"]["dilation"] == 3 and by["aspp_d3"]["pad"] == 3
    assert "dilation" not in by["aspp_1x1"] and "dilation" not in by["stem"]           # an ordinary conv's dict is what it was
    assert (by["dec_up1"]["align_corners"], by["dec_up1"]["align_mode"]) == (False, 1)
    assert by["dec_up2"]["align_corners"] is False and by["logits_up"]["align_corners"] is True
    assert by["logits"]["act"] == 0 and (by["label"]["axis"], by["label"]["dtype"], by["label"]["keepdims"]) == (1, -1, False)
    big = wl.seg_mini_net(res=512, num_classes=21)["shapes"]
    assert big["logits"] == (21, 256, 256) and big["label"] == (512, 512) and big["enc3_pw"] == (64, 64, 64)


def test_lowering_of_seg_mini_net(lite, wl, segnet):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dump_interp_plans as D
    golden = D.load_fixtures()
    assert len(golden) == 6
    nofuse = _plan(lite, wl, segnet, fuse=False)
    _check_unfused(nofuse, segnet)
    assert _heads(nofuse).count("bilinear_interp/def") == 2 and _heads(nofuse).count("nearest_interp/def") == 1 and _heads(nofuse).count("arg_max/def") == 1
    off = _plan(lite, wl, segnet, fuse=True, fuse_interp_argmax=False, fuse_interp_calib=False)
    assert not [h for h in _heads(off) if h in ("arg_max/interp", "bilinear_interp/int8", "nearest_interp/int8")]
    assert _heads(off).count("concat/int8") == 2            # L takes both concats, whatever M and N do
    got = {}
    for tag, m, n in (("m_on", True, False), ("n_on", False, True), ("mn_on", True, True)):
        got[tag] = _plan(lite, wl, segnet, fuse=True, fuse_interp_argmax=m, fuse_interp_calib=n)
        want, took_m, took_n = _rule_mn(off, m, n)
        assert got[tag] == want, tag
        assert took_m == (["logits_up"] if m else []) and took_n == (["dec_up2"] if n else []), tag
        assert _plan(lite, wl, segnet, fuse=False, fuse_interp_argmax=m, fuse_interp_calib=n) == nofuse     # both need set_fuse(true)
    on = got["mn_on"]
    assert len(off) - len(on) == 2
    assert "bilinear_interp/def in=aspp_project out=dec_up1 size=16x16 align_corners=0 align_mode=1" in on      # feeds a concat: stays
    assert "nearest_interp/int8 in=dec_conv1 out=dec_up2 size=32x32 align_corners=0 align_mode=1 +calib=dec_up2/precision_trans scale=0.0314960629 -f32" in on
    assert ("arg_max/interp in=logits out=label +interp=bilinear_interp size=64x64 align_corners=1 align_mode=1 axis=1 dtype=-1 keepdims=0 "
            "via=logits_up") in on
    assert "logits_up" not in " ".join(l.split(" via=")[0] for l in on)       # the resampled logits are no variable any more
    default = _plan(lite, wl, segnet, fuse=True)
    assert default == on           # M and N are on by default (measured)
    for sw, pl in (("nofuse", nofuse), ("default", default), ("mn_off", off), ("m_on", got["m_on"]), ("n_on", got["n_on"]), ("mn_on", on)):
        assert pl == golden["seg_mini.%s.b2" % sw], sw
    # a fetch of the low-resolution logits changes nothing M looks at; a fetch of the resampled logits keeps the two instructions
    with_logits = _plan(lite, wl, segnet, fuse=True, fuse_interp_argmax=True, fuse_interp_calib=True, fetch=("logits",))
    assert [l for l in with_logits if not l.endswith("out=logits/host")] == on
    kept = _plan(lite, wl, segnet, fuse=True, fuse_interp_argmax=True, fuse_interp_calib=True, fetch=("logits_up",))
    assert "arg_max/def in=logits_up out=label axis=1 dtype=-1 keepdims=0" in kept and "arg_max/interp" not in _heads(kept)


def test_m_and_n_fire_only_on_their_patterns(lite):
    def head(p, axis=1, extra=None):
        _conv(p, "x", "c", 8, 8)
        p.graph_interp("bilinear_interp", "c", "up", (8, 8), 0.0, True, 1)
        p.graph_arg_max("up", "out", axis, 2, False)
        if extra:
            extra(p)
    m_line = "arg_max/interp in=c out=out +interp=bilinear_interp size=8x8 align_corners=1 align_mode=1 axis=1 dtype=2 keepdims=0 via=up"
    assert m_line in _mini(lite, head)
    assert m_line.replace("axis=1", "axis=-3") in _mini(lite, lambda p: head(p, -3))
    assert m_line in _mini(lite, head, m=None)                                                      # the builder's default
    for kw in (dict(m=False), dict(fuse=False)):
        assert "arg_max/interp" not in _heads(_mini(lite, head, **kw)), kw
    assert "arg_max/interp" not in _heads(_mini(lite, lambda p: head(p, 2)))                        # another axis
    assert "arg_max/interp" not in _heads(_mini(lite, head, fetch=("out", "up")))                   # the resampled tensor is fetched
    both = _mini(lite, lambda p: head(p, 1, lambda q: _conv(q, "up", "d", 8, 8)), fetch=("out", "d"))    # ... or read by a conv too: N takes it
    assert "arg_max/interp" not in _heads(both) and "arg_max/def in=up out=out axis=1 dtype=2 keepdims=0" in both
    assert "bilinear_interp/int8 in=c out=up size=8x8 align_corners=1 align_mode=1 +calib=up/precision_trans scale=0.0500000007" in both

    def dec(p, reader=True):
        p.graph_interp("nearest_interp", "x", "up", None, 2.0, False, 1)
        _conv(p, "up", "out", 8, 8)
        if reader:
            p.graph_pool("up", "pooled", "max", (2, 2), (2, 2), (0, 0, 0, 0), False, True, False)
    n_line = "nearest_interp/int8 in=x/target_trans out=up by=2 align_corners=0 align_mode=1 +calib=up/precision_trans scale=0.0500000007"
    assert n_line + " -f32" in _mini(lite, lambda p: dec(p, False))
    assert n_line in _mini(lite, dec, fetch=("out", "pooled"))              # an fp32 reader is left: the fp32 tensor is written too
    assert n_line + " -f32" in _mini(lite, lambda p: dec(p, False), n=None)
    for kw in (dict(n=False), dict(fuse=False)):
        assert "nearest_interp/int8" not in _heads(_mini(lite, lambda p: dec(p, False), **kw)), kw
    only_f32 = _mini(lite, lambda p: (p.graph_interp("bilinear_interp", "x", "up", (8, 8)),
                                      p.graph_pool("up", "out", "max", (2, 2), (2, 2), (0, 0, 0, 0), False, True, False)))
    assert "bilinear_interp/def in=x/target_trans out=up size=8x8 align_corners=1 align_mode=1" in only_f32


def test_no_plan_of_an_existing_workload_changes(lite, wl):
    nets = [wl.mobilenet_v1_net(), wl.mobilenet_v2_net(), wl.mobilenet_v3_net("large"), wl.mobilenet_v3_net("small"), wl.resnet50_net(),
            wl.resnext50_net(), wl.shufflenet_v2_net(), wl.squeezenet_v1_1_net(), wl.inception_mini_net()]
    for net in nets:
        for kw in (dict(), dict(fuse_hard_act=True)):
            base = _plan(lite, wl, net, **kw)
            assert _plan(lite, wl, net, fuse_interp_argmax=False, fuse_interp_calib=False, **kw) == base, net["output"]


# ------------------------------------------------------------------ health and the label margin, on the oracle alone
def test_seg_mini_net_is_as_healthy_as_mobilenet_v2_and_its_labels_are_decided(wl, plref, segnet):
    """The rule of test_squeezenet_host.py: the yardstick is the worst int8 tensor of mobilenet_v2_net (0.048 saturated, 0.637 zeros
    when that was written).  seg_mini_net on two images of seed 350: worst saturated share 0.014, worst zero share 0.560, over
    12 int8 tensors.
    The labels: a pixel whose two largest resampled logits are closer than 2e-5 * max|logit| may come out differently on a device
    whose logits differ in the last bits (tests/test_gpu_segnet.py excuses those, at most 1 %).  On the oracle 1 of 8192 pixels
    (0.012 %) is that close for the committed seed."""
    import oracle.graph_oracle as GO
    img = np.random.default_rng(350).uniform(-1, 1, (2, 3, 224, 224)).astype(F32)
    mb = {k: ((np.abs(v.astype(np.int32)) == 127).mean(), (v == 0).mean()) for k, v in GO.forward(plref, wl.mobilenet_v2_net(), img, via_gemm=True).items()
          if v.dtype == np.int8}
    worst_sat, worst_zero = max(v[0] for v in mb.values()), max(v[1] for v in mb.values())
    img64 = np.random.default_rng(350).uniform(-1, 1, (2, 3, 64, 64)).astype(F32)
    ref = I.forward(plref, segnet, img64)
    sh = {k: ((np.abs(v.astype(np.int32)) == 127).mean(), (v == 0).mean()) for k, v in ref.items() if v.dtype == np.int8}
    assert len(sh) == 12, sorted(sh)
    print("seg_mini: worst saturated %.4f (yardstick %.4f), worst zero %.4f (yardstick %.4f)" % (
        max(v[0] for v in sh.values()), worst_sat, max(v[1] for v in sh.values()), worst_zero))
    for name, (sat, zero) in sh.items():
        assert sat <= worst_sat and zero <= worst_zero, (name, sat, zero)
    lab, up, logits = ref["label"], ref["logits_up"], ref["logits"]
    assert lab.shape == (2, 64, 64) and lab.dtype == np.int64 and up.shape == (2, 19, 64, 64) and np.isfinite(up).all()
    assert np.array_equal(lab, I.arg_max(I.interp(logits, (64, 64), "bilinear", True, 1), 1))
    assert len(np.unique(lab)) >= 4                       # not one label everywhere
    top = np.sort(up, axis=1)
    close = (top[:, -1] - top[:, -2]) < 2e-5 * float(np.abs(logits).max())
    print("seg_mini: %d of %d pixels have their two largest logits within 2e-5 * max|logit|" % (close.sum(), close.size))
    assert close.mean() < 0.01
