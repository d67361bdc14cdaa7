"""-m gpu: workloads.ssd_mini_net (an SSD-shaped detector: four feature maps with loc / conf heads and prior boxes, the heads
joined by transpose -> reshape -> concat, box_coder, softmax, multiclass_nms on the device) as a whole program at res 96, batch 2 and
batch 3.  The programs with fusion O on, with O off, and with no graph-level fusion at all are bit-identical in every fetched and
device-read tensor; against detection_oracle.forward the int8 tensors and the prior boxes are exact, the decoded boxes and the class
probabilities within 1e-5, and the device's detections are EXACTLY the oracle's multiclass_nms applied to the DEVICE's own boxes
and probabilities: the chain that leaves nothing unexplained.  The symmetric difference to the oracle's own detections is printed,
not asserted: it hangs on 1e-5 differences at the two thresholds.  One replay through run_graph() into poisoned variables
gives the bytes run() gave."""
import importlib

import numpy as np
import pytest

import detection_oracle as D
import replay_cases as R

pytestmark = pytest.mark.gpu
F32 = np.float32
RES = 96
FETCH = ("boxes", "prob")
# read where they live, on the device (every program writes them): an int8 tensor in front of a head, the joined heads, the priors
DEVICE_VARS = (("b2_pw/precision_trans", np.int8), ("b4_pw/precision_trans", np.int8), ("loc", F32), ("conf", F32), ("priors", F32),
               ("prior_vars", F32))


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


@pytest.fixture(scope="module")
def ssdnet(wl):
    return wl.ssd_mini_net(res=RES)


@pytest.fixture(scope="module")
def oracle(plref, ssdnet):
    """batch -> (image, name -> tensor), computed once and left unchanged."""
    out = {}
    for batch in (2, 3):
        img = np.random.default_rng(360).uniform(-1, 1, (batch, 3, RES, RES)).astype(F32)
        out[batch] = (img, D.forward(plref, ssdnet, img))
    return out


def _run(lite, wl, net, img, replay=False, ctx=None, **kw):
    """Lowers and runs the net twice (replay: then once more as a launch graph); returns (name -> array, plan, kernel names)."""
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, img.shape[0], fetch=FETCH, **kw)
        plan = p.graph_plan()
        assert p.graph_lower() == [v + "/host" for v in FETCH] + ["det/count/host", out]
        assert p.num_instructions() == len(plan)
        p.set_input(net["input"], img)
        p.run()
        p.run()

        def read():
            got = {"det": p.get_var("det/host", F32), "det/count": p.get_var("det/count/host", np.int32)}
            got.update({v: p.get_var(v + "/host", F32) for v in FETCH})
            got.update({v: p.get_var(v, t) for v, t in DEVICE_VARS})
            return got
        got = read()
        if replay:
            # every variable the plan writes but the priors (made on the host once) is poisoned: the replay has to write them all
            names, kept = R.to_poison(plan, p.kernel_names())
            assert len(kept) == 17 and "det" in names and "det/count" in names and "priors" in names, kept
            before = R.read_bytes(p, names)
            p.run_graph()  # records (after a plain run of its own), then launches
            R.poison(p, ctx, names)
            p.run_graph()  # replays
            p.sync()
            again = {"det": p.get_var("det", F32), "det/count": p.get_var("det/count", np.int32)}
            assert again["det"].tobytes() == got["det"].tobytes() and again["det/count"].tobytes() == got["det/count"].tobytes()
            diff = R.first_difference(plan, R.read_bytes(p, names), before)
            assert diff is None, "the replayed launch graph differs from run(): " + diff
        lod = p.detections("det")
        return got, plan, p.kernel_names(), lod
    finally:
        p.close()


@pytest.mark.parametrize("batch", [2, 3])
def test_ssd_mini_net_against_the_oracle_and_between_the_programs(lite, wl, ssdnet, oracle, gpu_ctx, batch):
    img, ref = oracle[batch]
    on, plan_on, kernels_on, lod = _run(lite, wl, ssdnet, img, replay=True, ctx=gpu_ctx, fuse=True, fuse_detection_head=True)
    off, plan_off, kernels_off, _ = _run(lite, wl, ssdnet, img, fuse=True, fuse_detection_head=False)
    un, plan_un, _, _ = _run(lite, wl, ssdnet, img, fuse=False)
    heads = [l.split(" ")[0] for l in plan_on]
    assert heads.count("concat/nhwc") == 2 and heads.count("transpose/def") == 0 and heads.count("reshape/def") == 8
    assert heads.count("multiclass_nms/def") == 1 and "scores=npc via=scores" in [l for l in plan_on if l.startswith("multiclass_nms")][0]
    assert len(plan_off) - len(plan_on) == 17  # 2 x (4 transposes + 4 reshapes) and the transpose in front of the NMS
    assert [l.split(" ")[0] for l in plan_off].count("transpose/def") == 9
    assert not [l for l in plan_off + plan_un if l.startswith("concat/nhwc") or "scores=npc" in l]
    names = "\n".join(kernels_on)
    for part in ("/nhwc -> concat_nhwc_hip", "/def -> multiclass_nms_npc_hip", "/def -> box_coder_decode_hip", "/def -> prior_box_host_once",
                 "/def -> reshape_share"):
        assert part in names, (part, names)
    assert "/def -> transpose_hip" in "\n".join(kernels_off) and "/def -> multiclass_nms_hip" in "\n".join(kernels_off)
    for v in on:
        assert on[v].tobytes() == off[v].tobytes(), v + ": O on differs from O off"
        assert on[v].tobytes() == un[v].tobytes(), v + ": O on differs from the unfused program"
    # against the oracle: int8 and the host-made priors exactly, fp32 within the project's rule
    for v in ("b2_pw/precision_trans", "b4_pw/precision_trans"):
        assert on[v].shape == ref[v].shape and np.array_equal(on[v], ref[v]), "%s: %d of %d int8 values differ" % (v, (on[v] != ref[v]).sum(), ref[v].size)
    for v in ("priors", "prior_vars"):
        assert on[v].shape == ref[v].shape and on[v].tobytes() == ref[v].tobytes(), v
    for v in ("loc", "conf", "boxes", "prob"):
        assert on[v].shape == ref[v].shape, v
        np.testing.assert_allclose(on[v], ref[v], rtol=1e-5, atol=1e-5, err_msg=v)
    # the NMS itself is exact: the oracle's multiclass_nms on the boxes and probabilities the DEVICE made
    nms = [o for o in ssdnet["ops"] if o["op"] == "multiclass_nms"][0]
    want = D.nms_padded(on["boxes"], np.ascontiguousarray(on["prob"].transpose(0, 2, 1)), nms)
    assert on["det/count"].tolist() == want["/count"].tolist()
    assert on["det"].shape == (batch, 200, 6) and on["det"].tobytes() == want[""].tobytes()
    assert all(s["kept"] > 200 and s["suppressed"] > 0 for s in want["/stats"])
    # the LoD form of the fetched result
    rows, offsets, idx = lod
    assert idx is None and offsets.tolist() == [0] + np.cumsum(want["/count"]).tolist() and rows.shape == (offsets[-1], 6)
    assert rows.tobytes() == np.concatenate([want[""][i, :want["/count"][i]] for i in range(batch)]).tobytes()
    # against the oracle's own detections: printed, not asserted
    mine = {tuple(r) for i in range(batch) for r in np.round(on["det"][i, :on["det/count"][i]], 4).tolist()}
    theirs = {tuple(r) for i in range(batch) for r in np.round(ref["det"][i, :ref["det/count"][i]], 4).tolist()}
    print("ssd_mini batch %d: %d detections, %d not among the oracle's own %d" % (batch, len(mine), len(mine - theirs), len(theirs)))
