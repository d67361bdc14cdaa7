"""CPU tests of the YOLOv3 heads above the C ABI: the two kernel classes' registrations, YoloBoxParam (a field-for-field subset of the
reference's; yolo_compute.cc compiles against the reference's own struct text), GraphBuilder's shape rule for yolo_box and every
fatal case, the int32 feed that lowering leaves alone, fusion P's pattern and every negative case of it, the plan fixtures of
yolov3_mini_net, the unchanged plans of every existing workload, and the structure and health of the synthetic net on the CPU
oracle."""
import importlib
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import yolo_oracle as Y

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITE = os.path.join(ROOT, "paddle-lite_amd")
REFERENCE = "/root/reference"
A3 = [10, 13, 16, 30, 33, 23]


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


@pytest.fixture(scope="module")
def yolonet(wl):
    return wl.yolov3_mini_net()


def _heads(plan):
    return [l.split(" ")[0] for l in plan]


# ------------------------------------------------------------------ registration, struct
def test_plugin_symbols_are_exported_and_the_kernels_registered(lite):
    LL = lite.load()
    for name in ("pllite_graph_yolo_box", "pllite_graph_set_fuse_yolo_head"):
        assert hasattr(LL, name), name
    for name in ("graph_yolo_box", "graph_set_fuse_yolo_head"):
        assert hasattr(lite.Predictor, name), name
    assert lite.PREC_INT32 == 3
    assert LL.pllite_registered_kernels(b"yolo_box", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 2      # def and head
    src = open(os.path.join(LITE, "lite", "kernels", "hip", "yolo_compute.cc")).read()
    assert re.findall(r"REGISTER_LITE_KERNEL\((\w+), kHIP, (\w+), (\w+), [\w:]+, (\w+)\)", src) == [
        ("yolo_box", "kFloat", "kNCHW", "def"), ("yolo_box", "kFloat", "kNCHW", "head")]
    assert src.count('BindInput("ImgSize", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt32))})') == 2
    assert '"yolo_box_hip"' in src and '"yolo_head_hip"' in src   # what kernel_names() reports


def test_the_param_struct_is_the_reference_struct_field_for_field():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_ref_params_header as g
    ours = g.struct_text(open(os.path.join(LITE, "lite", "operators", "op_params.h")).read(), "YoloBoxParam")
    fields = re.findall(r"^\s+(?:const\s+)?[\w:<>\s\*]+?[\s\*&](\w+)\s*(?:\{[^}]*\})?;", ours, re.M)
    assert fields == ["X", "ImgSize", "Boxes", "Scores", "anchors", "class_num", "conf_thresh", "downsample_ratio", "clip_bbox", "scale_x_y"]
    assert "YoloBoxParam" in g.STRUCTS
    side = open(os.path.join(LITE, "lite", "kernels", "hip", "yolo_fusion.h")).read()
    assert "struct HipYoloHead" in side and "HipYoloHeadKernel" in side and "downsample_ratio" in side
    if not os.path.isdir(os.path.join(REFERENCE, "lite")):
        return  # the reference tree is not on this machine: the two comparisons against its text cannot be made
    theirs = g.struct_text(open(os.path.join(REFERENCE, "lite", "operators", "op_params.h")).read(), "YoloBoxParam")
    decl = lambda text: [re.sub(r"\s+", " ", l.strip()) for l in text.splitlines()[1:-1] if l.strip() and not l.strip().startswith("//")]  # noqa: E731
    assert decl(ours) == decl(theirs)
    with tempfile.TemporaryDirectory(prefix="khip_refparams.") as tmp:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_ref_params_header.py"), "--out", tmp], stdout=subprocess.DEVNULL)
        assert "struct YoloBoxParam" in open(os.path.join(tmp, "lite", "operators", "op_params.h")).read()
        p = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", tmp, "-I", LITE, "-I", os.path.join(ROOT, "include"),
                            os.path.join(LITE, "lite", "kernels", "hip", "yolo_compute.cc")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "yolo_compute.cc does not compile against the reference's struct:\n%s" % p.stdout.decode()[-3000:]


# ------------------------------------------------------------------ InferShapes, the int32 feed, the fatal cases
def _conv(p, src, dst, cin, cout, in_scale=0.05):
    w = np.ones((cout, cin, 1, 1), np.int8)
    p.graph_conv("conv2d", src, dst, w, None, (1, 1), (0, 0, 0, 0), (1, 1), 1, 0, 0.0, in_scale, np.full(cout, 0.01, F32))


def _nms(p, boxes, scores, dst="out"):
    p.graph_multiclass_nms(boxes, scores, dst, background_label=-1, score_threshold=0.01, nms_top_k=400, nms_threshold=0.45, keep_top_k=20, normalized=False)


def _mini(lite, build, fetch=("out",), fuse=True, p_on=True, feed=(2, 8, 4, 6), img=(2, 2), img_prec=None):
    """A planner graph: feeds x (fp32) and img (int32) -> build(p) -> the fetches."""
    p = lite.Predictor(planner=True)
    try:
        p.graph_set_fuse(fuse)
        if p_on is not None:
            p.graph_set_fuse_yolo_head(p_on)
        p.graph_feed("x", feed)
        p.graph_feed("img", img, lite.PREC_INT32 if img_prec is None else img_prec)
        build(p)
        for f in fetch:
            p.graph_fetch(f)
        return p.graph_plan()
    finally:
        p.close()


def _yolo(p, src, tag, anchors=A3, class_num=3, conf_thresh=0.01, ratio=32, clip=True, sxy=1.0, img="img"):
    p.graph_yolo_box(src, img, tag + "_b", tag + "_s", anchors, class_num, conf_thresh, ratio, clip, sxy)


def _three(p, order=(0, 1, 2), **kw):
    """Three head convs on x (24 channels: 3 anchors x (5 + 3)), a yolo_box each, the joins and the NMS."""
    for i in range(3):
        _conv(p, "x", "h%d" % i, 8, 24)
        _yolo(p, "h%d" % i, "y%d" % i, ratio=32 >> i, **(kw if i == 1 else {}))
    p.graph_concat(["y0_b", "y1_b", "y2_b"], "boxes", 1)
    p.graph_concat(["y%d_s" % i for i in order], "scores_npc", 1)
    p.graph_transpose("scores_npc", "scores", (0, 2, 1))
    _nms(p, "boxes", "scores")


def test_infer_shapes_and_the_fatal_cases(lite):
    """concat CHECKs that its operands differ along the axis only, so a concat that plans proves the shapes InferShapes gave."""
    def sizes_ok(p):
        _conv(p, "x", "h", 8, 24)
        _yolo(p, "h", "y")                                              # Boxes [2, 72, 4], Scores [2, 72, 3]
        p.graph_reshape("h", "r", (2, 72, -1))                          # [2, 72, 16]
        p.graph_concat(["y_b", "y_s", "r"], "out", 2)                   # [2, 72, 23]: plans only if P = 3 * 4 * 6 = 72
    plan = _mini(lite, sizes_ok, p_on=False)
    assert ("yolo_box/def in=h,img/target_trans out=y_b,y_s anchors=10,13,16,30,33,23 class_num=3 conf_thresh=0.00999999978 downsample_ratio=32 "
            "clip_bbox=1 scale_x_y=1") in plan
    # the int32 operand: an io_copy, no calib; the head conv in front of an fp32 op takes the fp32_out kernel
    assert "io_copy/host_to_device in=img out=img/target_trans" in plan and not [l for l in plan if l.startswith("calib") and "img" in l]
    assert [l for l in plan if l.startswith("conv2d")][0].startswith("conv2d/fp32_out in=x/precision_trans out=h")

    def fatal(words, build, **kw):
        with pytest.raises(lite.LiteError) as e:
            _mini(lite, build, fetch=("out_b",), **kw)
        assert words in str(e.value), str(e.value)
    head = lambda p, c=24: _conv(p, "x", "h", 8, c)  # noqa: E731
    fatal("X must be [N, C, H, W]", lambda p: (head(p), p.graph_reshape("h", "r", (0, 24, -1)), _yolo(p, "r", "out")))
    fatal("anchors must hold (width, height) pairs, has 0", lambda p: (head(p), _yolo(p, "h", "out", anchors=[])))
    fatal("anchors must hold (width, height) pairs, has 3", lambda p: (head(p), _yolo(p, "h", "out", anchors=[10, 13, 16])))
    fatal("class_num 0 must be positive", lambda p: (head(p), _yolo(p, "h", "out", class_num=0)))
    fatal("X has 24 channels, 3 anchors of 4 classes need 27", lambda p: (head(p), _yolo(p, "h", "out", class_num=4)))
    fatal("X has 25 channels", lambda p: (head(p, 25), _yolo(p, "h", "out")))
    fatal("ImgSize must be [2, 2]", lambda p: (head(p), _yolo(p, "h", "out")), img=(3, 2))
    fatal("ImgSize must be [2, 2]", lambda p: (head(p), _yolo(p, "h", "out")), img=(2, 3))
    fatal("ImgSize must be [2, 2]", lambda p: (head(p), _yolo(p, "h", "out")), img=(2, 2, 1))
    fatal("is not produced by an earlier op or feed", lambda p: (head(p), _yolo(p, "h", "out", img="nowhere")))


# ------------------------------------------------------------------ fusion P
def test_p_fires_on_its_pattern(lite):
    on = _mini(lite, _three)
    line = ("yolo_box/head in=h0,img/target_trans,h1,h2 out=boxes,scores anchors=10,13,16,30,33,23|10,13,16,30,33,23|10,13,16,30,33,23 class_num=3 "
            "conf_thresh=0.00999999978 downsample_ratio=32|16|8 clip_bbox=1 scale_x_y=1 via=y0_b,y0_s,y1_b,y1_s,y2_b,y2_s,scores_npc")
    assert line in on and _heads(on).count("yolo_box/head") == 1
    assert not {"yolo_box/def", "concat/def", "transpose/def"} & set(_heads(on))
    assert [l for l in on if l.startswith("multiclass_nms")][0].startswith("multiclass_nms/def in=boxes,scores out=out,out/count ")
    assert "scores=npc" not in " ".join(on)
    # the head stands where the last yolo_box stood: behind every head conv
    assert _heads(on).index("yolo_box/head") > max(i for i, h in enumerate(_heads(on)) if h.startswith("conv2d"))
    off = _mini(lite, _three, p_on=False)
    assert len(off) - len(on) == 4 and _heads(off).count("yolo_box/def") == 3 and _heads(off).count("concat/def") == 2
    assert "transpose/def" not in _heads(off) and "scores=npc via=scores" in [l for l in off if l.startswith("multiclass_nms")][0]   # O2 still folds
    un = _mini(lite, _three, fuse=False)
    assert _mini(lite, _three, fuse=False, p_on=False) == un and "yolo_box/head" not in _heads(un)         # with set_fuse(true) only
    assert _heads(un).count("transpose/def") == 1 and _heads(un).count("yolo_box/def") == 3
    # k = 1: one yolo_box without concats whose Scores go through the transpose
    def one(p):
        _conv(p, "x", "h", 8, 24)
        _yolo(p, "h", "y")
        p.graph_transpose("y_s", "scores", (0, 2, 1))
        _nms(p, "y_b", "scores")
    k1 = _mini(lite, one)
    assert [l for l in k1 if l.startswith("yolo_box")] == [
        "yolo_box/head in=h,img/target_trans out=y_b,scores anchors=10,13,16,30,33,23 class_num=3 conf_thresh=0.00999999978 downsample_ratio=32 "
        "clip_bbox=1 scale_x_y=1 via=y_s"]
    assert "transpose/def" not in _heads(k1)


def test_p_leaves_every_other_shape_of_graph_alone(lite):
    """Each negative case keeps three yolo_box/def instructions and both concats."""
    def kept(build, **kw):
        plan = _mini(lite, build, **kw)
        assert "yolo_box/head" not in _heads(plan) and _heads(plan).count("yolo_box/def") == 3 and _heads(plan).count("concat/def") >= 2, plan
        return plan
    kept(_three, fetch=("out", "y1_s"))                                    # a fetched link
    kept(_three, fetch=("out", "y1_b"))
    kept(_three, fetch=("out", "scores_npc"))
    kept(_three, fetch=("out", "boxes"))
    kept(_three, fetch=("out", "scores"))
    kept(lambda p: (_three(p), p.graph_concat(["y2_s", "y2_s"], "second", 1)), fetch=("out", "second"))   # a second reader
    kept(lambda p: (_three(p), p.graph_concat(["boxes", "boxes"], "second", 1)), fetch=("out", "second"))
    kept(lambda p: _three(p, conf_thresh=0.02))                            # differing attributes
    kept(lambda p: _three(p, class_num=3, clip=False))
    kept(lambda p: _three(p, sxy=1.05))
    kept(lambda p: _three(p, order=(0, 2, 1)))                             # scores concatenated in another order
    kept(lambda p: _three(p, order=(1, 0, 2)))

    def other_img(p):
        p.graph_feed("img2", (2, 2), lite.PREC_INT32)
        _three(p, img="img2")
    kept(other_img)                                                        # another ImgSize

    def other_perm(p):
        for i in range(3):
            _conv(p, "x", "h%d" % i, 8, 24)
            _yolo(p, "h%d" % i, "y%d" % i)
        p.graph_concat(["y0_b", "y1_b", "y2_b"], "boxes", 1)
        p.graph_concat(["y0_s", "y1_s", "y2_s"], "s", 1)
        p.graph_reshape("s", "scores", (0, 3, -1))                         # a reshape is no transpose
        _nms(p, "boxes", "scores")
    kept(other_perm)


# ------------------------------------------------------------------ the workload's plans
def test_lowering_of_yolov3_mini_net(lite, wl, yolonet):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dump_yolo_plans as T
    golden = T.load_fixtures()
    assert len(golden) == 4
    got = T.plans(sys.modules["paddle_lite_amd"])
    for name in golden:
        assert got[name] == golden[name], name
    nofuse, default, off, on = (golden["yolov3_mini.%s.b2" % s] for s in ("nofuse", "default", "p_off", "p_on"))
    assert default == on                       # P is on by default (measured)
    assert _heads(nofuse).count("yolo_box/def") == 3 and _heads(nofuse).count("concat/def") == 4 and _heads(nofuse).count("transpose/def") == 1
    assert _heads(nofuse).count("nearest_interp/def") == 2 and _heads(nofuse).count("elementwise_add/def") == 5
    # the unfused program against the oracle's plan: every calib and every kernel pick
    want = Y.plan(yolonet)
    body = nofuse[2:-2]
    assert nofuse[:2] == ["io_copy/host_to_device in=image out=image/target_trans", "io_copy/host_to_device in=img_size out=img_size/target_trans"]
    assert len(body) == len(want)
    feeds = (yolonet["input"], yolonet["img_size"])
    for line, (kind, s) in zip(body, want):
        head, toks = line.split(" ")[0], line.split(" ")
        if kind == "calib":
            src = s["src"] + ("/target_trans" if s["src"] in feeds else "")
            assert head == "calib/fp32_to_int8" and ("in=" + src) in toks and ("out=" + s["dst"]) in toks, line
            continue
        o = s["o"]
        name = {"add": "elementwise_add"}.get(o["op"], o["op"])
        alias = ("int8_out" if s["int8_out"] else "fp32_out") if o["op"] == "conv2d" else "def"
        ins = [v + ("/target_trans" if v in feeds else "") for v in s["ins"]]
        assert head == name + "/" + alias and ("in=" + ",".join(ins)) in toks and ("out=" + ",".join(Y.outs_of(o))) in toks, line
    assert len(off) - len(on) == 4
    assert [l for l in on if l.startswith("yolo_box")] == [
        "yolo_box/head in=y32_head,img_size/target_trans,y16_head,y8_head out=boxes,scores anchors=27,21,36,46,86,75|7,14,14,10,14,27|2,3,4,7,8,5 "
        "class_num=20 conf_thresh=0.00999999978 downsample_ratio=32|16|8 clip_bbox=1 scale_x_y=1 via=y32_boxes,y32_scores,y16_boxes,y16_scores,"
        "y8_boxes,y8_scores,scores_npc"]
    assert on[-3].startswith("multiclass_nms/def in=boxes,scores out=det,det/count background=-1 ") and "normalized=0" in on[-3]
    assert on[-2:] == ["io_copy/device_to_host in=det/count out=det/count/host", "io_copy/device_to_host in=det out=det/host"]
    assert [l for l in off if l.startswith("multiclass_nms")][0].endswith("scores=npc via=scores")


def test_no_plan_of_an_existing_workload_changes(lite, wl, pkg):
    """Every plan fixture of the existing workloads is regenerated and found unchanged; and the new switch changes no plan of a
    network without a yolo_box."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    for tool in ("dump_plans", "dump_concat_plans", "dump_interp_plans", "dump_detection_plans", "dump_deconv_plans"):
        t = importlib.import_module(tool)
        golden, got = t.load_fixtures(), t.plans(pkg)
        assert sorted(golden) == sorted(got) and golden, tool
        for name in golden:
            assert got[name] == golden[name], (tool, name)

    def plan(net, **kw):
        p = lite.Predictor(planner=True)
        try:
            wl.emit_graph(p, net, 2, **kw)
            return p.graph_plan()
        finally:
            p.close()
    for net in (wl.mobilenet_v1_net(), wl.squeezenet_v1_1_net(), wl.seg_mini_net(), wl.ssd_mini_net(), wl.unet_mini_net()):
        assert plan(net, fuse_yolo_head=True) == plan(net) == plan(net, fuse_yolo_head=False), net["output"]


# ------------------------------------------------------------------ structure and health, on the oracle alone
def test_structure_of_yolov3_mini_net(wl, yolonet):
    ops, sh = yolonet["ops"], yolonet["shapes"]
    assert yolonet["input_shape"] == (3, 96, 96) and yolonet["output"] == "det" and yolonet["img_size"] == "img_size" and sh["det"] == (100, 6)
    assert sh["s3_res"] == (64, 12, 12) and sh["s4_res"] == (96, 6, 6) and sh["s5_res"] == (128, 3, 3)
    assert [sh[t + "_head"] for t in ("y32", "y16", "y8")] == [(75, 3, 3), (75, 6, 6), (75, 12, 12)]
    assert [sh[t + "_boxes"] for t in ("y32", "y16", "y8")] == [(27, 4), (108, 4), (432, 4)] and sh["y8_scores"] == (432, 20)
    assert sh["boxes"] == (567, 4) and sh["scores_npc"] == (567, 20) and sh["scores"] == (20, 567)
    by = {o["name"]: o for o in ops}
    assert all(o["act"] == 4 and abs(o["act_coef"] - 0.1) < 1e-7 for o in ops if o["op"] == "conv2d" and not o["name"].endswith("_head"))
    assert all(by[t + "_head"]["act"] == 0 and by[t + "_head"]["w"].shape[2:] == (1, 1) for t in ("y32", "y16", "y8"))
    assert all(by["s%d_res" % i]["act"] == "" for i in range(1, 6)) and all(by["s%d_down" % i]["stride"] == 2 for i in range(1, 6))
    assert by["n32_up"]["op"] == "nearest_interp" and (by["n32_up"]["out_h"], by["n16_up"]["out_h"]) == (6, 12)
    assert by["n16_cat"]["srcs"] == ["n32_up", "s4_res"] and by["n8_cat"]["srcs"] == ["n16_up", "s3_res"]
    ys = [o for o in ops if o["op"] == "yolo_box"]
    assert [o["downsample_ratio"] for o in ys] == [32, 16, 8] and all(o["conf_thresh"] == 0.01 and o["clip_bbox"] and o["scale_x_y"] == 1.0 for o in ys)
    assert sum((o["anchors"] for o in reversed(ys)), ()) == tuple(int(round(a * 96 / 416.0)) or 1 for a in wl.COCO_ANCHORS)
    assert by["boxes"]["srcs"] == ["y32_boxes", "y16_boxes", "y8_boxes"] and by["scores_npc"]["srcs"] == ["y32_scores", "y16_scores", "y8_scores"]
    assert by["scores"]["perm"] == (0, 2, 1)
    n = by["det"]
    assert (n["background_label"], n["score_threshold"], n["nms_top_k"], n["nms_threshold"], n["keep_top_k"], n["normalized"], n["nms_eta"]) == (
        -1, 0.01, 400, 0.45, 100, False, 1.0)
    big = wl.yolov3_mini_net(res=416, num_classes=80)["shapes"]
    assert big["boxes"] == (10647, 4) and big["scores"] == (80, 10647) and big["y8_head"] == (255, 52, 52)


def test_yolov3_mini_net_gives_the_head_and_the_nms_work_to_do(wl, plref, yolonet):
    """Two images of seed 361 on the CPU oracle (committed seed, obj_shift 1.4, head_range 6).  Of the 567 cells of an image a clear
    share falls on each side of conf_thresh; the NMS keeps more than keep_top_k boxes before the cut (so the cut to 100 is
    exercised) and suppresses candidates by overlap in every image.  The int8 tensors are within test_squeezenet_host.py's yardstick
    (mobilenet_v2_net's worst tensor: 0.048 saturated, 0.637 zeros).  The figures are DESIGN.md 16's."""
    rng = np.random.default_rng(361)
    feeds = {"image": rng.uniform(-1, 1, (2, 3, 96, 96)).astype(F32), "img_size": np.array([[96, 96], [240, 320]], np.int32)}
    ref = Y.forward(plref, yolonet, feeds)
    kept_cells = sum(ref[t + "_boxes/parts"]["keep"].sum(axis=1) for t in ("y32", "y16", "y8"))
    stats = ref["det/stats"]
    print("yolov3_mini: cells kept of 567", kept_cells.tolist(), stats, ref["det/count"].tolist())
    for t in ("y32", "y16", "y8"):
        Y.assert_clear_of_threshold(ref[t + "_boxes/parts"], t)
    assert all(0.2 * 567 < k < 0.8 * 567 for k in kept_cells)         # 1. a clear share of cells on each side of the threshold
    assert all(s["kept"] > 100 for s in stats)                         # 2. the keep_top_k cut is exercised
    assert all(s["suppressed"] > 0 for s in stats)                     # 3. overlap suppresses in every image
    assert ref["det/count"].tolist() == [100, 100]
    det = ref["det"]
    assert det.shape == (2, 100, 6) and (np.diff(det[0, :, 0]) >= 0).all() and det[:, :, 0].min() >= 0 and det[:, :, 0].max() <= 19
    assert np.isfinite(ref["boxes"]).all() and ref["boxes"].shape == (2, 567, 4) and ref["scores"].shape == (2, 20, 567)
    # the clip bounds the near corners below and the far corners above, nothing else
    assert ref["boxes"][0, :, 2:].max() <= 95 and ref["boxes"][1, :, 2].max() <= 319 and ref["boxes"][1, :, 3].max() <= 239 and ref["boxes"][:, :, :2].min() >= 0
    i8 = {k: ((np.abs(v.astype(np.int32)) == 127).mean(), (v == 0).mean()) for k, v in ref.items() if getattr(v, "dtype", None) == np.int8}
    assert len(i8) == 22, sorted(i8)
    print("yolov3_mini: worst saturated %.4f, worst zero %.4f" % (max(v[0] for v in i8.values()), max(v[1] for v in i8.values())))
    for name, (sat, zero) in i8.items():
        assert sat <= 0.048 and zero <= 0.637, (name, sat, zero)
