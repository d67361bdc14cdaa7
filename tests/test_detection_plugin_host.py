"""CPU tests of the detection heads above the C ABI: the kernel classes' registrations, the param structs (subsets of the reference's,
and detection_compute.cc compiles against the reference's own struct text), the host prior_box function compiled into a stand-alone
program against detection_oracle bit for bit, liteapi.detections_lod against the oracle, GraphBuilder's shape rules and every fatal
case, fusion O's two patterns and what they must leave alone, the plan fixtures of ssd_mini_net, the unchanged plans of every
existing workload, and the structure and health of the synthetic net on the CPU oracle."""
import importlib
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import detection_oracle as D

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITE = os.path.join(ROOT, "paddle-lite_amd")
PARAMS = (("ReshapeParam", 7), ("TransposeParam", 6), ("BoxCoderParam", 8), ("MulticlassNmsParam", 11), ("PriorBoxParam", 18))


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


@pytest.fixture(scope="module")
def ssdnet(wl):
    return wl.ssd_mini_net()


# ------------------------------------------------------------------ registration, structs
def test_plugin_symbols_are_exported_and_the_kernels_registered(lite):
    LL = lite.load()
    ops = ("transpose", "reshape", "prior_box", "box_coder", "multiclass_nms")
    for name in ["pllite_add_" + o for o in ops] + ["pllite_graph_" + o for o in ops] + ["pllite_add_concat_nhwc", "pllite_graph_set_fuse_detection_head"]:
        assert hasattr(LL, name), name
    for name in ["add_" + o for o in ops] + ["graph_" + o for o in ops] + ["add_concat_nhwc", "graph_set_fuse_detection_head", "detections"]:
        assert hasattr(lite.Predictor, name), name
    for op in ops + ("transpose2", "reshape2"):
        assert LL.pllite_registered_kernels(op.encode(), lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1, op
    # concat/nhwc is registered at the layout it writes: concat/def stays the one kernel a pick at NCHW finds
    assert LL.pllite_registered_kernels(b"concat", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1
    src = open(os.path.join(LITE, "lite", "kernels", "hip", "detection_compute.cc")).read()
    assert re.findall(r"REGISTER_LITE_KERNEL\((\w+), kHIP, (\w+), (\w+), [\w:]+, (\w+)\)", src) == [
        ("concat", "kFloat", "kNHWC", "nhwc"), ("transpose", "kFloat", "kNCHW", "def"), ("transpose2", "kFloat", "kNCHW", "def"),
        ("reshape", "kFloat", "kNCHW", "def"), ("reshape2", "kFloat", "kNCHW", "def"), ("prior_box", "kFloat", "kNCHW", "def"),
        ("box_coder", "kFloat", "kNCHW", "def"), ("multiclass_nms", "kFloat", "kNCHW", "def")]


@pytest.mark.skipif(not os.path.isdir("/root/reference/lite"), reason="reference tree not present on this machine")
def test_detection_compute_compiles_against_the_reference_param_structs():
    """The method of test_boundary_reference_params.py: the generated header holds the reference's own struct text, and the count
    tensor lives in the side header."""
    with tempfile.TemporaryDirectory(prefix="khip_refparams.") as tmp:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_ref_params_header.py"), "--out", tmp], stdout=subprocess.DEVNULL)
        gen = open(os.path.join(tmp, "lite", "operators", "op_params.h")).read()
        for name, _ in PARAMS:
            assert "struct " + name in gen, name
        assert "count" not in re.search(r"struct MulticlassNmsParam.*?\n};", gen, re.S).group(0)
        side = open(os.path.join(LITE, "lite", "kernels", "hip", "detection_fusion.h")).read()
        assert "lite::Tensor* count" in side and "scores_npc" in side and "HipNmsFusionKernel" in side
        p = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", tmp, "-I", LITE, "-I", os.path.join(ROOT, "include"),
                            os.path.join(LITE, "lite", "kernels", "hip", "detection_compute.cc")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "detection_compute.cc does not compile against the reference's structs:\n%s" % p.stdout.decode()[-3000:]


@pytest.mark.skipif(not os.path.isdir("/root/reference/lite"), reason="reference tree not present on this machine")
def test_the_param_structs_are_subsets_of_the_reference_fields():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_ref_params_header as g
    ref = open("/root/reference/lite/operators/op_params.h").read()
    ours = open(os.path.join(LITE, "lite", "operators", "op_params.h")).read()
    for name, n_fields in PARAMS:
        mine, theirs = g.struct_text(ours, name), g.struct_text(ref, name)
        fields = re.findall(r"^\s+(?:const\s+)?[\w:<>\s\*]+?[\s\*&](\w+)\s*(?:\{[^}]*\})?;", mine, re.M)
        assert len(fields) == n_fields, (name, fields)
        missing = [f for f in fields if not re.search(r"\b%s\b" % f, theirs)]
        assert not missing, "%s has fields the reference lacks: %s" % (name, missing)


# ------------------------------------------------------------------ prior_box: the host function, stand-alone, against the oracle
PRIOR_CASES = [
    # (feat h, w, image h, w, min_sizes, max_sizes, aspect_ratios, flip, clip, step_w, step_h, offset, min_max_aspect_ratios_order)
    (12, 12, 96, 96, [19.2], [41.6], [2.0], 1, 0, 0.0, 0.0, 0.5, 0),
    (6, 6, 96, 96, [41.6], [64.0], [2.0, 3.0], 1, 0, 0.0, 0.0, 0.5, 0),
    (1, 1, 96, 96, [86.4], [96.0], [2.0], 1, 1, 0.0, 0.0, 0.5, 1),
    (19, 19, 300, 300, [60.0], [105.0], [2.0, 3.0], 1, 1, 16.0, 16.0, 0.5, 1),
    (5, 7, 301, 299, [30.0, 60.0], [], [1.0, 2.0, 2.0000001, 0.5], 0, 0, 0.0, 0.0, 0.25, 0),
    (3, 2, 64, 100, [8.0, 20.5], [16.9, 33.0], [], 1, 0, 0.0, 8.0, 0.5, 0),
]
PRIOR_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "lite/kernels/hip/prior_box_host.h"
// argv: h w img_h img_w flip clip step_w step_h offset order n_min min.. n_max max.. n_ar ar..; stdout: the raw floats, boxes then variances
int main(int argc, char** argv) {
  int a = 1;
  const int h = atoi(argv[a++]), w = atoi(argv[a++]), ih = atoi(argv[a++]), iw = atoi(argv[a++]), flip = atoi(argv[a++]), clip = atoi(argv[a++]);
  const float sw = strtof(argv[a++], nullptr), sh = strtof(argv[a++], nullptr), off = strtof(argv[a++], nullptr);
  const int order = atoi(argv[a++]);
  std::vector<float> v[3];
  for (auto& l : v) {
    const int n = atoi(argv[a++]);
    for (int i = 0; i < n; ++i) l.push_back(strtof(argv[a++], nullptr));
  }
  std::vector<float> boxes, vars;
  paddle::lite::kernels::hip::PriorBoxHost(h, w, ih, iw, v[0], v[1], v[2], flip != 0, clip != 0, {0.1f, 0.1f, 0.2f, 0.2f}, sw, sh, off, order != 0,
                                          &boxes, &vars);
  if ((int)boxes.size() != h * w * 4 * paddle::lite::kernels::hip::PriorBoxNum(v[0], v[1], v[2], flip != 0)) return 3;
  fwrite(boxes.data(), sizeof(float), boxes.size(), stdout);
  fwrite(vars.data(), sizeof(float), vars.size(), stdout);
  return 0;
}
"""


def test_prior_box_host_function_equals_the_oracle_bit_for_bit():
    with tempfile.TemporaryDirectory(prefix="khip_priorbox.") as tmp:
        src, exe = os.path.join(tmp, "main.cc"), os.path.join(tmp, "prior_box")
        open(src, "w").write(PRIOR_MAIN)
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-I", LITE, src, "-o", exe])
        for h, w, ih, iw, mins, maxs, ars, flip, clip, sw, sh, off, order in PRIOR_CASES:
            args = [h, w, ih, iw, flip, clip, repr(sw), repr(sh), repr(off), order, len(mins)] + [repr(v) for v in mins] + \
                   [len(maxs)] + [repr(v) for v in maxs] + [len(ars)] + [repr(v) for v in ars]
            raw = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, check=True).stdout
            want_b, want_v = D.prior_box((h, w), (ih, iw), mins, maxs, ars, (0.1, 0.1, 0.2, 0.2), bool(flip), bool(clip), sw, sh, off, bool(order))
            got = np.frombuffer(raw, F32)
            assert got.size == 2 * want_b.size, (h, w, got.size, want_b.shape)
            assert got[:want_b.size].tobytes() == want_b.tobytes(), ("boxes", h, w, mins)
            assert got[want_b.size:].tobytes() == want_v.tobytes(), ("variances", h, w, mins)
    # by hand: one cell of a 1 x 1 map of a 100 x 100 image, min 20, max 80, ratio 2 with flip: 20; 20 sqrt 2 x 20 / sqrt 2 and its
    # flip; sqrt(1600) = 40, centred at 50
    b, v = D.prior_box((1, 1), (100, 100), [20], [80], [2.0])
    assert b.shape == (1, 1, 4, 4) and np.array_equal(b[0, 0, 0], np.array([0.4, 0.4, 0.6, 0.6], F32)) and np.array_equal(b[0, 0, 3], np.array([0.3, 0.3, 0.7, 0.7], F32))
    r = F32(20) * np.sqrt(F32(2))
    assert b[0, 0, 1, 0] == (F32(50) - r / F32(2)) / F32(100) and b[0, 0, 2, 1] == (F32(50) - r / F32(2)) / F32(100)
    assert np.array_equal(v[0, 0], np.tile(np.array([0.1, 0.1, 0.2, 0.2], F32), (4, 1)))
    assert np.array_equal(D.prior_box((1, 1), (100, 100), [20], [80], [2.0], min_max_aspect_ratios_order=True)[0][0, 0, 1], b[0, 0, 3])
    assert [float(a) for a in D.expand_aspect_ratios([1.0, 2.0, 2.0, 0.5], True)] == [1.0, 2.0, 0.5]
    assert [float(a) for a in D.expand_aspect_ratios([2.0, 0.5], False)] == [1.0, 2.0, 0.5]


def test_detections_lod_of_the_api_equals_the_oracle(lite):
    boxes, scores, params, (rows, offsets, index, _stats) = D.random_case((3, 5, 300))
    po, pc, pi = D.padded(rows, offsets, index, params["keep_top_k"])
    for idx in (pi, None):
        got, want = lite.detections_lod(po, pc, idx), D.detections_lod(po, pc, idx)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist() == offsets.tolist()
        assert (got[2] is None and want[2] is None) if idx is None else (got[2].tolist() == want[2].tolist() == index[:, None].tolist())
    none = np.full((2, 4, 6), -1, F32)
    r, o, i = lite.detections_lod(none, [0, 0])
    assert r.tolist() == [[-1.0]] and o.tolist() == [0, 1] and i is None
    r, o, i = lite.detections_lod(none, [0, 0], np.full((2, 4), -1, np.int32))
    assert r.shape == (0, 6) and o.tolist() == [0, 0, 0] and i.shape == (0, 1) and i.dtype == np.int32
    one = none.copy()
    one[1, 0] = [3, 0.5, 0, 0, 1, 1]
    r, o, i = lite.detections_lod(one, [0, 1], np.array([[-1] * 4, [9, -1, -1, -1]], np.int32))
    assert r.tolist() == [one[1, 0].tolist()] and o.tolist() == [0, 0, 1] and i.tolist() == [[9]]
    for bad in (([0, 5],), ([0],), ([-1, 0],)):
        with pytest.raises(ValueError):
            lite.detections_lod(none, *bad)


# ------------------------------------------------------------------ InferShapes and the fatal cases
def _mini(lite, build, fetch=("out",), fuse=True, o=True, feed=(2, 8, 4, 6)):
    """A planner graph: feed x -> build(p) -> the fetches."""
    p = lite.Predictor(planner=True)
    try:
        p.graph_set_fuse(fuse)
        if o is not None:
            p.graph_set_fuse_detection_head(o)
        p.graph_feed("x", feed)
        build(p)
        for f in fetch:
            p.graph_fetch(f)
        return p.graph_plan()
    finally:
        p.close()


def _heads(plan):
    return [l.split(" ")[0] for l in plan]


def _nms(p, boxes, scores, dst="out", **kw):
    args = dict(background_label=0, score_threshold=0.01, nms_top_k=400, nms_threshold=0.45, keep_top_k=20)
    args.update(kw)
    p.graph_multiclass_nms(boxes, scores, dst, **args)


def test_infer_shapes_and_the_fatal_cases(lite):
    """concat CHECKs that its operands differ along the axis only, so a concat that plans proves the shapes InferShapes gave."""
    def sizes(p):
        p.graph_transpose("x", "t", (0, 2, 3, 1))                       # [2, 4, 6, 8]
        p.graph_reshape("t", "r", (0, -1, 4))                           # [2, 48, 4]
        p.graph_reshape("x", "r2", (0, 0, 4, 6))                        # [2, 8, 4, 6]: every 0 copies
        p.graph_transpose("r2", "t2", (0, 1, 3, 2))                     # [2, 8, 6, 4]
        p.graph_reshape("t2", "r3", (2, 48, -1))                        # [2, 48, 4]
        p.graph_concat(["r", "r3"], "boxes", 1)                         # [2, 96, 4]
        p.graph_prior_box("x", "x", "pb", "pv", [2.0], [3.0], [2.0])    # [4, 6, 4, 4] each
        p.graph_reshape("pb", "pbf", (-1, 4))                           # [96, 4]
        p.graph_reshape("pv", "pvf", (-1, 4))
        p.graph_box_coder("pbf", "boxes", "dec", prior_var="pvf")       # [2, 96, 4]
        p.graph_box_coder("pb", "boxes", "dec2", variance=[0.1, 0.1, 0.2, 0.2])   # the 4-D prior_box output as it is
        p.graph_concat(["dec", "dec2"], "both", 2)                      # [2, 96, 8]
        p.graph_transpose("both", "sc", (0, 2, 1))                      # [2, 8, 96]
        _nms(p, "dec", "sc", "out", index="idx")                       # [2, 20, 6], [2], [2, 20]
        p.graph_transpose("idx", "idx_t", (1, 0))                       # [20, 2]
        p.graph_reshape("out/count", "cnt", (1, 2))                     # [1, 2]
        p.graph_concat(["idx_t", "cnt"], "out2", 0)                     # [21, 2]
    plan = _mini(lite, sizes, fetch=("out", "out2"), o=False)
    assert "transpose/def in=x/target_trans out=t perm=0,2,3,1" in plan and "reshape/def in=t out=r shape=0,-1,4" in plan
    assert ("prior_box/def in=x/target_trans,x/target_trans out=pb,pv min_sizes=2 max_sizes=3 aspect_ratios=2 variances=0.100000001,0.100000001,"
            "0.200000003,0.200000003 flip=1 clip=0 step_w=0 step_h=0 offset=0.5 min_max_aspect_ratios_order=0") in plan
    assert "box_coder/def in=pbf,pvf,boxes out=dec code_type=decode_center_size axis=0 normalized=1" in plan
    assert "box_coder/def in=pb,boxes out=dec2 code_type=decode_center_size axis=0 normalized=1 variance=0.100000001,0.100000001,0.200000003,0.200000003" in plan
    assert ("multiclass_nms/def in=dec,sc out=out,out/count,idx background=0 score_threshold=0.00999999978 nms_top_k=400 nms_threshold=0.449999988 "
            "nms_eta=1 keep_top_k=20 normalized=1 count=out/count") in plan

    def fatal(words, build, **kw):
        with pytest.raises(lite.LiteError) as e:
            _mini(lite, build, **kw)
        assert words in str(e.value), str(e.value)
    fatal("not a permutation", lambda p: p.graph_transpose("x", "out", (0, 1, 1, 3)))
    fatal("not a permutation", lambda p: p.graph_transpose("x", "out", (0, 1, 2, 4)))
    fatal("entries for rank", lambda p: p.graph_transpose("x", "out", (0, 2, 1)))
    fatal("outside 2 .. 4", lambda p: (p.graph_reshape("x", "r", (2, 2, 4, 4, 6)), p.graph_transpose("r", "out", (0, 1, 2, 3, 4))))
    fatal("more than one -1", lambda p: p.graph_reshape("x", "out", (0, -1, -1)))
    fatal("another count", lambda p: p.graph_reshape("x", "out", (2, 8, 5, 5)))
    fatal("does not divide", lambda p: p.graph_reshape("x", "out", (0, -1, 5)))
    fatal("beyond the input's rank", lambda p: p.graph_reshape("x", "out", (2, 8, 4, 3, 0)))
    fatal("in the shape", lambda p: p.graph_reshape("x", "out", (2, -8, 4, 6)))
    fatal("one max_size per min_size", lambda p: p.graph_prior_box("x", "x", "out", "v", [2.0, 4.0], [3.0]))
    fatal("min_sizes", lambda p: p.graph_prior_box("x", "x", "out", "v", []))
    ok = lambda p: (p.graph_transpose("x", "t", (0, 2, 3, 1)), p.graph_reshape("t", "b", (0, -1, 4)), p.graph_reshape("t", "s", (0, 8, -1)))  # noqa: E731
    fatal("PriorBox must be [48, 4]", lambda p: (ok(p), p.graph_reshape("x", "pr", (-1, 4)), p.graph_box_coder("pr", "b", "out")))
    fatal("PriorBoxVar must have", lambda p: (ok(p), p.graph_reshape("b", "pr", (-1, 4)), p.graph_concat(["pr", "pr"], "pv", 0),
                                               p.graph_box_coder("pr", "b", "out", prior_var="pv")), feed=(1, 8, 4, 6))
    fatal("TargetBox must be", lambda p: (p.graph_reshape("x", "pr", (-1, 4)), p.graph_box_coder("pr", "x", "out")))
    fatal("axis 2", lambda p: (ok(p), p.graph_reshape("b", "pr", (-1, 4)), p.graph_box_coder("pr", "b", "out", axis=2)), feed=(1, 8, 4, 6))
    with pytest.raises(ValueError, match="variance"):                       # the C API takes exactly four: refused in front of it
        _mini(lite, lambda p: (ok(p), p.graph_reshape("b", "pr", (-1, 4)), p.graph_box_coder("pr", "b", "out", variance=[0.1, 0.2])), feed=(1, 8, 4, 6))
    with pytest.raises(ValueError, match="variances"):
        _mini(lite, lambda p: p.graph_prior_box("x", "x", "out", "v", [2.0], variance=[0.1]))
    fatal("disagree in N or P", lambda p: (ok(p), p.graph_transpose("s", "s2", (0, 2, 1)), _nms(p, "b", "s2")))       # scores [2, 24, 8]
    fatal("BBoxes must be [N, P, 4]", lambda p: (ok(p), _nms(p, "s", "s")))
    fatal("3-D score form", lambda p: (ok(p), _nms(p, "b", "x")))
    fatal("keep_top_k", lambda p: (ok(p), p.graph_reshape("t", "s3", (0, 4, 48)), _nms(p, "b", "s3", keep_top_k=-1)))
    fatal("keep_top_k", lambda p: (ok(p), p.graph_reshape("t", "s3", (0, 4, 48)), _nms(p, "b", "s3", keep_top_k=0)))
    fatal("nms_eta", lambda p: (ok(p), p.graph_reshape("t", "s3", (0, 4, 48)), _nms(p, "b", "s3", nms_eta=0.9)))
    # the envelope: P 16385; min(nms_top_k, P) 4097; classes * min(..) above 16384
    big = lambda p, pr, c: (p.graph_reshape("x", "b", (1, pr, 4)), p.graph_reshape("x", "s", (1, c, pr)))  # noqa: E731
    fatal("envelope", lambda p: (big(p, 16385, 4), _nms(p, "b", "s")), feed=(1, 4, 16385, 1))
    fatal("envelope", lambda p: (big(p, 8192, 4), _nms(p, "b", "s", nms_top_k=-1)), feed=(1, 4, 8192, 1))
    fatal("envelope", lambda p: (p.graph_split("x", ["x4", "rest"], 1, 0, (4, 4096)), p.graph_reshape("x4", "b", (1, 8, 4)), p.graph_reshape("x", "s", (1, 4100, 8)),
                                 _nms(p, "b", "s", nms_top_k=-1, background_label=-1)), feed=(1, 4100, 8, 1))       # 4100 classes x 8 lists
    inside = _mini(lite, lambda p: (big(p, 16384, 4), _nms(p, "b", "s", nms_top_k=4096, keep_top_k=4096)), feed=(1, 4, 16384, 1))
    assert "multiclass_nms/def" in _heads(inside)


# ------------------------------------------------------------------ fusion O
def _conv(p, src, dst, cin, cout, in_scale=0.05):
    w = np.ones((cout, cin, 3, 3), np.int8)
    p.graph_conv("conv2d", src, dst, w, None, (1, 1), (1, 1, 1, 1), (1, 1), 1, 0, 0.0, in_scale, np.full(cout, 0.01, F32))


def _head(p, perm=(0, 2, 3, 1), shape=(0, -1, 4), shape2=(0, -1, 4), extra=None, plain=False, axis=1):
    _conv(p, "x", "a", 8, 8)
    _conv(p, "x", "b", 8, 16)
    p.graph_transpose("a", "a_t", perm)
    p.graph_reshape("a_t", "a_r", shape)
    if plain:
        p.graph_reshape("b", "b_r", (0, -1, 4))
    else:
        p.graph_transpose("b", "b_t", (0, 2, 3, 1))
        p.graph_reshape("b_t", "b_r", shape2)
    if extra:
        extra(p)
    p.graph_concat(["a_r", "b_r"], "out", axis)


def test_o1_fires_only_on_its_pattern(lite):
    line = "concat/nhwc in=a,b out=out k=4 via=a_t,a_r,b_t,b_r"
    on = _mini(lite, _head)
    assert line in on and "transpose/def" not in _heads(on) and "reshape/def" not in _heads(on)
    off = _mini(lite, _head, o=False)
    assert len(off) - len(on) == 4 and _heads(off).count("transpose/def") == 2 and "concat/def in=a_r,b_r out=out axis=1" in off
    assert line.replace("axis=1", "axis=1") in _mini(lite, lambda p: _head(p, axis=-2))
    assert _mini(lite, _head, o=None) == on                                        # the builder's default: on (measured)
    assert _mini(lite, _head, fuse=False) == _mini(lite, _head, fuse=False, o=False)   # with set_fuse(true) only
    one = _mini(lite, lambda p: (_conv(p, "x", "a", 8, 8), p.graph_transpose("a", "a_t", (0, 2, 3, 1)), p.graph_reshape("a_t", "a_r", (0, -1, 8)),
                                 p.graph_concat(["a_r"], "out", 1)))
    assert "concat/nhwc in=a out=out k=8 via=a_t,a_r" in one                       # one operand
    for name, kw in (("a second reader of the transposed tensor", dict(extra=lambda p: p.graph_reshape("a_t", "other", (0, -1, 2)))),
                     ("another perm", dict(perm=(0, 3, 2, 1))), ("another shape", dict(shape=(2, -1, 4))), ("two k", dict(shape2=(0, -1, 8), axis=1)),
                     ("one plain operand", dict(plain=True))):
        if name == "two k":
            with pytest.raises(lite.LiteError):          # [2, 48, 4] and [2, 48, 8] do not concat along axis 1 at all
                _mini(lite, lambda p: _head(p, **kw))
            continue
        fetch = ("out", "other") if "second reader" in name else ("out",)
        plan = _mini(lite, lambda p, kw=kw: _head(p, **kw), fetch=fetch)
        assert "concat/nhwc" not in _heads(plan) and "concat/def in=a_r,b_r out=out axis=1" in plan, name
    for fetched in ("a_t", "a_r"):                                                  # a fetched link
        plan = _mini(lite, _head, fetch=("out", fetched))
        assert "concat/nhwc" not in _heads(plan), fetched
    # a concat along another axis of such chains
    def same(p):
        for v in ("a", "b"):
            _conv(p, "x", v, 8, 8)
            p.graph_transpose(v, v + "_t", (0, 2, 3, 1))
            p.graph_reshape(v + "_t", v + "_r", (0, -1, 4))
        p.graph_concat(["a_r", "b_r"], "out", 2)
    plan = _mini(lite, same)
    assert "concat/nhwc" not in _heads(plan)
    # the same chain twice as operands: its links have two uses
    twice = _mini(lite, lambda p: (_conv(p, "x", "a", 8, 8), p.graph_transpose("a", "a_t", (0, 2, 3, 1)), p.graph_reshape("a_t", "a_r", (0, -1, 4)),
                                   p.graph_concat(["a_r", "a_r"], "out", 1)))
    assert "concat/nhwc" not in _heads(twice)


def test_o2_fires_only_on_its_pattern(lite):
    def tail(p, perm=(0, 2, 1), extra=None, boxes_from_scores=False):
        p.graph_reshape("x", "b", (0, -1, 4))           # [2, 48, 4]
        p.graph_reshape("x", "s", (0, 48, -1))          # [2, 48, 4]: P 48, C 4
        if perm == (0, 2, 1):
            p.graph_transpose("s", "s_t", perm)         # [2, 4, 48]
        else:
            p.graph_reshape("s", "s_t", (0, 4, 48))
        if extra:
            extra(p)
        _nms(p, "b", "s_t")
    on = _mini(lite, tail)
    line = [l for l in on if l.startswith("multiclass_nms/def")][0]
    assert line.startswith("multiclass_nms/def in=b,s out=out,out/count ") and line.endswith(" count=out/count scores=npc via=s_t")
    assert "transpose/def" not in _heads(on)
    off = _mini(lite, tail, o=False)
    assert len(off) - len(on) == 1 and "transpose/def in=s out=s_t perm=0,2,1" in off and "scores=npc" not in " ".join(off)
    assert _mini(lite, tail, o=None) == on and "scores=npc" not in " ".join(_mini(lite, tail, fuse=False))
    assert "scores=npc" not in " ".join(_mini(lite, tail, fetch=("out", "s_t")))                             # the transposed scores are fetched
    second = _mini(lite, lambda p: tail(p, extra=lambda q: q.graph_softmax("s_t", "other")), fetch=("out", "other"))
    assert "scores=npc" not in " ".join(second) and "transpose/def in=s out=s_t perm=0,2,1" in second          # a second reader
    assert "scores=npc" not in " ".join(_mini(lite, lambda p: tail(p, perm=None)))                            # no transpose in front
    # a transpose in front of the BOXES operand is none of O2's business
    boxes_t = _mini(lite, lambda p: (p.graph_reshape("x", "bt", (0, 4, -1)), p.graph_transpose("bt", "b", (0, 2, 1)), p.graph_reshape("x", "s", (0, 4, 48)),
                                     _nms(p, "b", "s")))
    assert "transpose/def in=bt out=b perm=0,2,1" in boxes_t and "scores=npc" not in " ".join(boxes_t)


# ------------------------------------------------------------------ the lowering of ssd_mini_net, and every other workload's
def _plan(lite, wl, net, batch=2, **kw):
    p = lite.Predictor(planner=True)
    try:
        wl.emit_graph(p, net, batch, **kw)
        return p.graph_plan()
    finally:
        p.close()


def test_lowering_of_ssd_mini_net(lite, wl, ssdnet):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dump_detection_plans as T
    golden = T.load_fixtures()
    assert len(golden) == 4
    got = T.plans(sys.modules["paddle_lite_amd"])
    for name in golden:
        assert got[name] == golden[name], name
    nofuse, default, off, on = (golden["ssd_mini.%s.b2" % s] for s in ("nofuse", "default", "o_off", "o_on"))
    assert default == on                       # O is on by default (measured)
    assert _heads(nofuse).count("transpose/def") == 9 and _heads(nofuse).count("reshape/def") == 16 and _heads(nofuse).count("concat/def") == 4
    assert _heads(nofuse).count("prior_box/def") == 4 and _heads(nofuse).count("box_coder/def") == 1 and _heads(nofuse).count("softmax/def") == 1
    # the unfused program against the oracle's plan: every calib and every kernel pick
    want = D.plan(ssdnet)
    body = nofuse[1:-2]
    assert len(body) == len(want)
    for line, (kind, s) in zip(body, want):
        head, toks = line.split(" ")[0], line.split(" ")
        if kind == "calib":
            src = s["src"] + ("/target_trans" if s["src"] == ssdnet["input"] else "")
            assert head == "calib/fp32_to_int8" and ("in=" + src) in toks and ("out=" + s["dst"]) in toks, line
            continue
        o = s["o"]
        alias = ("int8_out" if s["int8_out"] else "fp32_out") if o["op"] in ("conv2d", "depthwise_conv2d") else "def"
        ins = [v + ("/target_trans" if v == ssdnet["input"] else "") for v in s["ins"]]
        assert head == o["op"] + "/" + alias and ("in=" + ",".join(ins)) in toks and ("out=" + ",".join(D.outs_of(o))) in toks, line
    # a feature map has an fp32 reader (its prior_box): fp32_out with the calib taken over by the conv
    assert "conv2d/fp32_out in=b2_dw out=b2_pw +calib=b2_pw/precision_trans scale=0.0314960629" in on
    assert len(off) - len(on) == 17 and _heads(on).count("concat/nhwc") == 2 and "transpose/def" not in _heads(on)
    assert ("concat/nhwc in=f0_conf,f1_conf,f2_conf,f3_conf out=conf k=21 via=f0_conf_nhwc,f0_conf_flat,f1_conf_nhwc,f1_conf_flat,f2_conf_nhwc,"
            "f2_conf_flat,f3_conf_nhwc,f3_conf_flat") in on
    assert "concat/def in=f0_prior_flat,f1_prior_flat,f2_prior_flat,f3_prior_flat out=priors axis=0" in on      # no transposes: not O's
    assert [l for l in on if l.startswith("multiclass_nms")][0].endswith("keep_top_k=200 normalized=1 count=det/count scores=npc via=scores")
    assert on[-2:] == ["io_copy/device_to_host in=det/count out=det/count/host", "io_copy/device_to_host in=det out=det/host"]
    # fetching the probabilities changes nothing O2 looks at; fetching the transposed scores keeps the transpose
    with_prob = _plan(lite, wl, ssdnet, fuse_detection_head=True, fetch=("prob",))
    assert [l for l in with_prob if not l.endswith("out=prob/host")] == on
    kept = _plan(lite, wl, ssdnet, fuse_detection_head=True, fetch=("scores",))
    assert "transpose/def in=prob out=scores perm=0,2,1" in kept and "scores=npc" not in " ".join(kept)


def test_no_plan_of_an_existing_workload_changes(lite, wl, pkg):
    """Every plan fixture of the existing workloads is regenerated and found unchanged; and the new switch changes no plan of a
    network without a transpose."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    for tool in ("dump_plans", "dump_concat_plans", "dump_interp_plans"):
        t = importlib.import_module(tool)
        golden, got = t.load_fixtures(), t.plans(pkg)
        assert sorted(golden) == sorted(got) and golden, tool
        for name in golden:
            assert got[name] == golden[name], (tool, name)
    for net in (wl.mobilenet_v1_net(), wl.mobilenet_v2_net(), wl.shufflenet_v2_net(), wl.squeezenet_v1_1_net(), wl.inception_mini_net(), wl.seg_mini_net()):
        assert _plan(lite, wl, net, fuse_detection_head=True) == _plan(lite, wl, net), net["output"]


# ------------------------------------------------------------------ structure and health, on the oracle alone
def test_structure_of_ssd_mini_net(wl, ssdnet):
    ops, sh = ssdnet["ops"], ssdnet["shapes"]
    assert ssdnet["input_shape"] == (3, 96, 96) and ssdnet["output"] == "det" and sh["det"] == (200, 6)
    assert sh["b2_pw"] == (64, 12, 12) and sh["b3_pw"] == (128, 6, 6) and sh["b4_pw"] == (128, 3, 3) and sh["extra"] == (64, 1, 1)
    assert [sh["f%d_loc" % k] for k in range(4)] == [(16, 12, 12), (24, 6, 6), (24, 3, 3), (16, 1, 1)]
    assert [sh["f%d_conf" % k][0] for k in range(4)] == [84, 126, 126, 84]
    assert sh["f1_prior"] == (6, 6, 6, 4) and sh["priors"] == (850, 4) and sh["prior_vars"] == (850, 4)
    assert sh["loc"] == (850, 4) and sh["conf"] == (850, 21) and sh["boxes"] == (850, 4) and sh["prob"] == (850, 21) and sh["scores"] == (21, 850)
    by = {o["name"]: o for o in ops}
    assert by["f0_loc"]["act"] == 0 and by["f0_conf"]["act"] == 0 and by["f0_conf"]["pad"] == 1 and by["extra"]["pad"] == 0
    assert by["f0_prior"]["aspect_ratios"] == (2.0,) and by["f1_prior"]["aspect_ratios"] == (2.0, 3.0) and by["f0_prior"]["flip"]
    assert abs(by["f0_prior"]["min_sizes"][0] - 19.2) < 1e-9 and by["f3_prior"]["max_sizes"] == (96.0,)
    assert by["boxes"]["prior_var"] == "prior_vars" and by["boxes"]["axis"] == 0 and by["scores"]["perm"] == (0, 2, 1)
    n = by["det"]
    assert (n["background_label"], n["score_threshold"], n["nms_top_k"], n["nms_threshold"], n["keep_top_k"], n["normalized"], n["nms_eta"]) == (
        0, 0.01, 400, 0.45, 200, True, 1.0)
    big = wl.ssd_mini_net(res=320)["shapes"]
    assert big["b2_pw"] == (64, 40, 40) and big["extra"] == (64, 8, 8) and big["priors"] == (40 * 40 * 4 + 20 * 20 * 6 + 10 * 10 * 6 + 8 * 8 * 4, 4)


def test_ssd_mini_net_gives_the_nms_work_to_do(wl, plref, ssdnet):
    """Two images of seed 360 on the CPU oracle.  What the NMS sees, per image (committed seed, conf_range 12): 3185 and 3188 boxes
    kept before the keep_top_k cut (so the cut to 200 is exercised), 3550 and 3572 candidates suppressed by overlap, and one
    foreground class (the last, whose biases are lowered) without a candidate; 7948 and 7996 of the 17000 foreground scores pass the
    threshold, and more than 400 do in some class, so nms_top_k cuts too.  The int8 tensors are as healthy as seg_mini_net's."""
    img = np.random.default_rng(360).uniform(-1, 1, (2, 3, 96, 96)).astype(F32)
    ref = D.forward(plref, ssdnet, img)
    stats = ref["det/stats"]
    print("ssd_mini:", stats, ref["det/count"].tolist(), (ref["scores"][:, 1:] > F32(0.01)).sum(axis=(1, 2)).tolist())
    assert max(s["kept"] for s in stats) > 200                       # 1. the cut is exercised
    assert all(s["suppressed"] > 0 for s in stats)                   # 2. overlap suppresses in every image
    assert max(s["empty_classes"] for s in stats) >= 1               # 3. a foreground class without a candidate
    assert ref["det/count"].tolist() == [200, 200] and (ref["scores"][:, 1:] > F32(0.01)).sum(axis=2).max() > 400
    assert not (ref["scores"][:, 20] > F32(0.01)).any()
    det = ref["det"]
    assert det.shape == (2, 200, 6) and (np.diff(det[0, :, 0]) >= 0).all() and det[:, :, 0].min() >= 1 and det[:, :, 0].max() <= 19
    assert np.isfinite(ref["boxes"]).all() and np.allclose(ref["prob"].sum(axis=2), 1, atol=1e-5)
    assert ref["priors"].shape == (850, 4) and ref["boxes"].shape == (2, 850, 4) and ref["prior_vars"][0].tolist() == [F32(0.1), F32(0.1), F32(0.2), F32(0.2)]
    i8 = {k: ((np.abs(v.astype(np.int32)) == 127).mean(), (v == 0).mean()) for k, v in ref.items() if getattr(v, "dtype", None) == np.int8}
    assert len(i8) == 11, sorted(i8)      # the image, the stem, 4 depthwise outputs, b1_pw and the calibs of the four feature maps
    print("ssd_mini: worst saturated %.4f, worst zero %.4f" % (max(v[0] for v in i8.values()), max(v[1] for v in i8.values())))
    for name, (sat, zero) in i8.items():
        assert sat <= 0.048 and zero <= 0.637, (name, sat, zero)     # test_squeezenet_host.py's yardstick: mobilenet_v2_net's worst tensor
