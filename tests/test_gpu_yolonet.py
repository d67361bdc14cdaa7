"""-m gpu: workloads.yolov3_mini_net (a YOLOv3-shaped detector: darknet-style residual backbone, an upsampling neck, three linear
heads, yolo_box per map, the boxes and scores joined by concat and transpose, multiclass_nms on the device) as a whole program at
res 96, batch 2 and batch 3, with a different ImgSize per image fed as int32.  The programs with fusion P on, with P off, and with
no graph-level fusion at all are bit-identical in every fetched and device-read tensor; against yolo_oracle.forward the int8 tensors
are exact and the fp32 head maps within 1e-5; the boxes and scores are within yolo_oracle's derived bounds of the oracle's yolo_box
applied to the DEVICE's own head maps; and the device's detections are EXACTLY detection_oracle.nms_padded applied to the
device's own boxes and scores.  The symmetric difference to the oracle's own detections is printed, not asserted.  One replay
through run_graph() into poisoned variables gives the bytes run() gave."""
import importlib

import numpy as np
import pytest

import detection_oracle as D
import replay_cases as R
import yolo_oracle as Y

pytestmark = pytest.mark.gpu
F32 = np.float32
RES = 96
HEADS = ("y32_head", "y16_head", "y8_head")
INT8_VARS = ("s3_res/precision_trans", "s5_a", "n16_cat/precision_trans", "n8")


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


@pytest.fixture(scope="module")
def yolonet(wl):
    return wl.yolov3_mini_net(res=RES)


def _feeds(batch):
    rng = np.random.default_rng(361)
    img = rng.uniform(-1, 1, (batch, 3, RES, RES)).astype(F32)
    size = np.array([[96, 96], [240, 320], [417, 353]], np.int32)[:batch]
    return {"image": img, "img_size": size}


@pytest.fixture(scope="module")
def oracle(plref, yolonet):
    """batch -> (feeds, name -> tensor), computed once and left unchanged."""
    return {batch: (_feeds(batch), Y.forward(plref, yolonet, _feeds(batch))) for batch in (2, 3)}


def _run(lite, wl, net, feeds, scores_var, replay=False, ctx=None, **kw):
    """Lowers and runs the net twice (replay: then once more as a launch graph); returns (name -> array, plan, kernel names, LoD)."""
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, feeds["image"].shape[0], **kw)
        plan = p.graph_plan()
        assert p.graph_lower() == ["det/count/host", out]
        assert p.num_instructions() == len(plan)
        for k, v in feeds.items():
            p.set_input(k, v)
        p.run()
        p.run()
        got = {"det": p.get_var("det/host", F32), "det/count": p.get_var("det/count/host", np.int32), "boxes": p.get_var("boxes", F32),
               scores_var: p.get_var(scores_var, F32)}
        got.update({v: p.get_var(v, F32) for v in HEADS})
        got.update({v: p.get_var(v, np.int8) for v in INT8_VARS})
        if replay:
            # every variable the plan writes is poisoned (the two feeds' device tensors are not the replay's to write)
            names, kept = R.to_poison(plan, p.kernel_names())
            assert sorted(kept) == ["image/target_trans", "img_size/target_trans"] and {"det", "det/count", "boxes", scores_var} <= set(names)
            before = R.read_bytes(p, names)
            p.run_graph()  # records (after a plain run of its own), then launches
            R.poison(p, ctx, names)
            p.run_graph()  # replays
            p.sync()
            diff = R.first_difference(plan, R.read_bytes(p, names), before)
            assert diff is None, "the replayed launch graph differs from run(): " + diff
            for v in ("det", "boxes", scores_var):
                assert p.get_var(v, F32).tobytes() == got[v].tobytes(), v + ": the replayed launch graph differs from run()"
            assert p.get_var("det/count", np.int32).tobytes() == got["det/count"].tobytes()
        return got, plan, p.kernel_names(), p.detections("det")
    finally:
        p.close()


@pytest.mark.parametrize("batch", [2, 3])
def test_yolov3_mini_net_against_the_oracle_and_between_the_programs(lite, wl, yolonet, oracle, gpu_ctx, batch):
    feeds, ref = oracle[batch]
    on, plan_on, kernels_on, lod = _run(lite, wl, yolonet, feeds, "scores", replay=True, ctx=gpu_ctx, fuse=True, fuse_yolo_head=True)
    off, plan_off, kernels_off, _ = _run(lite, wl, yolonet, feeds, "scores_npc", fuse=True, fuse_yolo_head=False)
    un, plan_un, _, _ = _run(lite, wl, yolonet, feeds, "scores", fuse=False)
    un2, _, _, _ = _run(lite, wl, yolonet, feeds, "scores_npc", fuse=False)
    # ---- the plans
    heads = [l.split(" ")[0] for l in plan_on]
    assert heads.count("yolo_box/head") == 1 and heads.count("yolo_box/def") == 0 and heads.count("transpose/def") == 0
    at = heads.index("yolo_box/head")
    assert "concat/def" not in heads[at:] and heads[at + 1:] == ["multiclass_nms/def", "io_copy/device_to_host", "io_copy/device_to_host"]
    assert len(plan_off) - len(plan_on) == 4 and [l.split(" ")[0] for l in plan_off].count("yolo_box/def") == 3
    assert "scores=npc via=scores" in [l for l in plan_off if l.startswith("multiclass_nms")][0]
    assert not [l for l in plan_off + plan_un if l.startswith("yolo_box/head")]
    assert [l for l in plan_on if "img_size" in l][0] == "io_copy/host_to_device in=img_size out=img_size/target_trans"
    assert not [l for l in plan_on + plan_un if l.startswith("calib") and "img_size" in l]
    assert "/head -> yolo_head_hip" in "\n".join(kernels_on) and "/def -> yolo_box_hip" not in "\n".join(kernels_on)
    assert "\n".join(kernels_off).count("/def -> yolo_box_hip") == 3 and "/def -> multiclass_nms_npc_hip" in "\n".join(kernels_off)
    # ---- P on, P off and fuse off: the same bytes
    for v in on:
        other = off if v != "scores" else un
        assert on[v].tobytes() == other[v].tobytes(), v + ": P on differs from " + ("P off" if v != "scores" else "the unfused program")
        if v != "scores":
            assert on[v].tobytes() == un2[v].tobytes(), v + ": P on differs from the unfused program"
    assert off["scores_npc"].tobytes() == un2["scores_npc"].tobytes()
    assert on["scores"].tobytes() == np.ascontiguousarray(off["scores_npc"].transpose(0, 2, 1)).tobytes()
    # ---- against the oracle: int8 exactly, the fp32 head maps within the project's rule
    for v in INT8_VARS:
        assert on[v].shape == ref[v].shape and np.array_equal(on[v], ref[v]), "%s: %d of %d int8 values differ" % (v, (on[v] != ref[v]).sum(), ref[v].size)
    for v in HEADS:
        assert on[v].shape == ref[v].shape, v
        np.testing.assert_allclose(on[v], ref[v], rtol=1e-5, atol=1e-5, err_msg=v)
    # ---- boxes and scores: the oracle's yolo_box on the DEVICE's own head maps, within the derived bounds
    ys = [o for o in yolonet["ops"] if o["op"] == "yolo_box"]
    assert [o["src"] for o in ys] == list(HEADS)
    wb, ws, pt = Y.yolo_head([on[v] for v in HEADS], feeds["img_size"], [o["anchors"] for o in ys], ys[0]["class_num"], ys[0]["conf_thresh"],
                             [o["downsample_ratio"] for o in ys], ys[0]["clip_bbox"], ys[0]["scale_x_y"], parts=True)
    assert on["boxes"].shape == (batch, 567, 4) and on["scores"].shape == (batch, 20, 567)
    worst = Y.check_against(on["boxes"], on["scores"], wb, ws, pt, "yolov3_mini batch %d" % batch, score_layout="ncp")
    print("yolov3_mini batch %d: worst box %.2f, worst score %.2f units of 2^-23 (bound 8); %s of 567 cells kept" % (
        (batch,) + worst + (pt["keep"].sum(axis=1).tolist(),)))
    assert all(0.1 * 567 < k < 0.9 * 567 for k in pt["keep"].sum(axis=1))
    # ---- the NMS itself is exact: the oracle's multiclass_nms on the boxes and scores the DEVICE made
    nms = [o for o in yolonet["ops"] if o["op"] == "multiclass_nms"][0]
    want = D.nms_padded(on["boxes"], on["scores"], nms)
    assert on["det/count"].tolist() == want["/count"].tolist()
    assert on["det"].shape == (batch, 100, 6) and on["det"].tobytes() == want[""].tobytes()
    assert all(s["kept"] > 100 and s["suppressed"] > 0 for s in want["/stats"])
    # ---- the LoD form of the fetched result
    rows, offsets, idx = lod
    assert idx is None and offsets.tolist() == [0] + np.cumsum(want["/count"]).tolist() and rows.shape == (offsets[-1], 6)
    assert rows.tobytes() == np.concatenate([want[""][i, :want["/count"][i]] for i in range(batch)]).tobytes()
    # ---- against the oracle's own detections: printed, not asserted
    mine = {tuple(r) for i in range(batch) for r in np.round(on["det"][i, :on["det/count"][i]], 3).tolist()}
    theirs = {tuple(r) for i in range(batch) for r in np.round(ref["det"][i, :ref["det/count"][i]], 3).tolist()}
    print("yolov3_mini batch %d: %d detections, %d not among the oracle's own %d" % (batch, len(mine), len(mine - theirs), len(theirs)))
