"""-m gpu: HipPredictor::RunGraph, the launch-graph path a serving loop and the benchmark's graph mode run a step through.  Every
program family is recorded on one input and REPLAYED on another that only the replay ever sees (uploaded through the io_copy
instructions alone), into variables filled with the poison byte; the replay must equal the plain run of a second predictor byte for
byte, twice (replay_cases.replay_equals_plain_run).  A replay that launches nothing, drops a node, skips an instruction whose
Launch() returns early, or runs a kernel that depends on what its output held before, fails here.  Then the stale-graph guard
(HipPredictor::GraphKey and the AddFeed mark), two graphs interleaved on one stream, and the error path.

No test can tell a replay from a silent re-record: the library exposes no counter."""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest

import replay_cases as R
from test_image_feed_host import BGR, MEANS, SCALES

pytestmark = pytest.mark.gpu
F32 = np.float32
NV12 = 12
FUSED_DWPW = "conv_depthwise_3x3_pointwise_1x1_fused_int8_hip"
FUSED_G = "conv_depthwise_3x3_conv1x1_fused_int8_hip"
GROUPED = "conv_grouped3x3_int8_mfma32x32x32"


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


def _tensor_feeds(net, seed, batch=2):
    rng = np.random.default_rng(seed)
    c, h, w = net["input_shape"]
    return [{net["input"]: rng.uniform(-1, 1, (batch, c, h, w)).astype(F32)} for _ in range(2)]


def _conv_workspace_bytes(pkg, net, batch):
    """name -> plhip_conv_workspace_bytes of every dense conv of the net at this batch."""
    capi = pkg.capi
    shapes = dict(net["shapes"])
    shapes[net["input"]] = net["input_shape"]
    out = {}
    for o in net["ops"]:
        if o["op"] != "conv2d":
            continue
        cin, h, w = shapes[o["src"]]
        cout, _, k, _ = o["w"].shape
        d = capi.conv_desc(batch, cin, h, w, cout, k, k, (o["pad"],) * 4, (o["stride"],) * 2, (o.get("dilation", 1),) * 2, o["groups"])
        out[o["name"]] = capi.load().plhip_conv_workspace_bytes(C.byref(d))
    return out


def _count(kernels, frag):
    return sum(frag in k for k in kernels)


# program -> (net, emit_graph keywords, feeds a / b, what must have run: checked on the kernel names and the plan)
def _mobilenet_v1(wl, pkg):
    net = wl.mobilenet_v1_net(seed=11)
    a, b = _tensor_feeds(net, 500)

    def check(kernels, plan):
        assert sum("+pw=" in l for l in plan) == 13 and _count(kernels, FUSED_DWPW) == 13, kernels
    return net, {}, a, b, check


def _mobilenet_v1_unfused_pairs(wl, pkg):
    net = wl.mobilenet_v1_net(seed=11)
    a, b = _tensor_feeds(net, 501)

    def check(kernels, plan):
        assert not any("+pw=" in l for l in plan) and _count(kernels, FUSED_DWPW) == 0
        assert sum(k.startswith("depthwise_conv2d") for k in kernels) == 13 and sum(k.startswith("conv2d") for k in kernels) == 14, kernels
        assert _count(kernels, "conv_depthwise_3x3_int8_int8_hip") == 13, kernels
    return net, dict(fuse_dwpw=False), a, b, check


def _mobilenet_v2(wl, pkg):
    net = wl.mobilenet_v2_net()
    a, b = _tensor_feeds(net, 502)

    def check(kernels, plan):
        assert _count(kernels, FUSED_G) == 17, kernels
    return net, dict(fuse_dwconv=True), a, b, check


def _resnet50(wl, pkg):
    net = wl.resnet50_net()
    a, b = _tensor_feeds(net, 503)

    def check(kernels, plan):
        ws = _conv_workspace_bytes(pkg, net, 2)
        assert sum(v > 0 for v in ws.values()) >= 16, ws      # the workspace routes (patch / implicit / im2col GEMM)
        assert sum("+add=" in l and "+relu" in l for l in plan) == 16   # the residual tails, inside the conv instructions
    return net, {}, a, b, check


def _resnext50(wl, pkg):
    net = wl.resnext50_net()
    a, b = _tensor_feeds(net, 504)

    def check(kernels, plan):
        assert _count(kernels, GROUPED) == 16, kernels
    return net, {}, a, b, check


def _mobilenet_v3_small(wl, pkg):
    net = wl.mobilenet_v3_net("small")
    a, b = _tensor_feeds(net, 505)

    def check(kernels, plan):
        assert _count(kernels, "se_gate_int8_dot4_hip") == 9 and _count(kernels, "se_scale_int8_hip") == 9, kernels
        assert _count(kernels, "hard_swish_int8_hip") > 0
    return net, dict(fuse_hard_act=True), a, b, check


def _shufflenet_v2(wl, pkg):
    net = wl.shufflenet_v2_net(0.5)
    a, b = _tensor_feeds(net, 506)

    def check(kernels, plan):
        assert _count(kernels, "shuffle_unit_int8_hip") == 13 and _count(kernels, "shuffle_concat_int8_hip") == 3, kernels
    return net, {}, a, b, check


def _squeezenet(wl, pkg):
    net = wl.squeezenet_v1_1_net()
    a, b = _tensor_feeds(net, 507)

    def check(kernels, plan):
        assert _count(kernels, "/int8 -> concat_int8_hip") == 8, kernels
        assert len([l for l in plan if l.startswith("pool2d/") and l.endswith(" int8")]) == 2, plan
    # this network's softmax runs over the last axis of [N, 1000, 1, 1]: prob is 1.0 whatever the image; pool10 in front of it tells
    # the two feeds apart
    return net, dict(probe="pool10"), a, b, check


def _inception_mini(wl, pkg):
    net = wl.inception_mini_net()
    a, b = _tensor_feeds(net, 508)

    def check(kernels, plan):
        assert any(l.startswith("concat/int8 ") for l in plan) and _count(kernels, "/int8 -> concat_") > 0, kernels
    return net, {}, a, b, check


def _seg_mini(wl, pkg):
    net = wl.seg_mini_net()
    a, b = _tensor_feeds(net, 509)

    def check(kernels, plan):
        assert _count(kernels, "/interp -> bilinear_interp_arg_max_hip") == 1 and _count(kernels, "/int8 -> nearest_interp_int8_hip") == 1, kernels
    return net, {}, a, b, check


def _unet_mini(wl, pkg):
    net = wl.unet_mini_net()
    a, b = _tensor_feeds(net, 510)

    def check(kernels, plan):
        assert _count(kernels, "deconv_phase_int8_mfma32x32x32") == 2, kernels
    return net, {}, a, b, check


def _ssd_mini(wl, pkg):
    net = wl.ssd_mini_net()
    a, b = _tensor_feeds(net, 511)

    def check(kernels, plan):
        for frag in ("/nhwc -> concat_nhwc_hip", "/def -> multiclass_nms_npc_hip", "/def -> prior_box_host_once", "/def -> reshape_share"):
            assert _count(kernels, frag) > 0, (frag, kernels)
        # 4 prior_box ops, two outputs and two reshape aliases each: kept, beside the feed
        assert len(R.once_outputs(plan)) == 16 and len(R.keep(plan, kernels)) == 17
    return net, dict(fuse_detection_head=True), a, b, check


def _yolov3_mini(wl, pkg):
    net = wl.yolov3_mini_net()
    a, b = _tensor_feeds(net, 512)
    a["img_size"] = np.array([[96, 96], [240, 320]], np.int32)
    b["img_size"] = np.array([[417, 353], [128, 96]], np.int32)

    def check(kernels, plan):
        assert _count(kernels, "/head -> yolo_head_hip") == 1 and len(R.feeds(plan)[0]) == 2, kernels
    return net, {}, a, b, check


def _mobilenet_v1_image_feed(wl, pkg):
    net = wl.mobilenet_v1_net(seed=11)
    rng = np.random.default_rng(513)
    a, b = [{net["input"]: rng.integers(0, 256, (2, 224, 224, 3)).astype(np.uint8)} for _ in range(2)]

    def check(kernels, plan):
        assert _count(kernels, "-> image_to_tensor_int8+") == 1 and " +image_in=image fmt=BGR " in plan[1], kernels[:3]
    return net, dict(image=dict(format=BGR, means=MEANS, scales=SCALES)), a, b, check


def _mobilenet_v1_nv12_frames(wl, pkg):
    net = wl.mobilenet_v1_net(seed=11)
    rng = np.random.default_rng(514)
    a, b = [{net["input"]: rng.integers(0, 256, (2, 96 * 3 // 2, 128)).astype(np.uint8)} for _ in range(2)]

    def check(kernels, plan):
        assert _count(kernels, "nv12_image_resize_to_tensor_int8_hip") == 1 and " src=NV12 96x128->224x224 " in plan[1], kernels[:3]
    return net, dict(frame=dict(h=96, w=128, format=NV12, means=MEANS, scales=SCALES)), a, b, check


PROGRAMS = [_mobilenet_v1, _mobilenet_v1_unfused_pairs, _mobilenet_v2, _resnet50, _resnext50, _mobilenet_v3_small, _shufflenet_v2, _squeezenet,
            _inception_mini, _seg_mini, _unet_mini, _ssd_mini, _yolov3_mini, _mobilenet_v1_image_feed, _mobilenet_v1_nv12_frames]


@pytest.mark.parametrize("program", PROGRAMS, ids=[f.__name__[1:] for f in PROGRAMS])
def test_replay_on_new_input_into_poisoned_variables_equals_the_plain_run(lite, wl, pkg, gpu_ctx, program):
    """Batch 2; the classification networks at 224 x 224 (no kernel list of a smaller resolution was compared with the one at 224, so
    none is used), the mini networks at their own resolution."""
    net, kw, feeds_a, feeds_b, check = program(wl, pkg)
    kw = dict(kw)
    probe = kw.pop("probe", None)
    kernels, plan = R.replay_equals_plain_run(lite, wl, gpu_ctx, net, feeds_a, feeds_b, program.__name__[1:], probe=probe, **kw)
    check(kernels, plan)


# ------------------------------------------------------------------ the stale-graph guard
def _poisoned_run_graph_equals(p, ctx, plan, names, want, what):
    """poison -> run_graph() -> compare, twice: where the first call drops a stale graph it records again (a plain run of its own
    comes first), and the second call replays what it recorded."""
    for call in ("first", "second"):
        R.poison(p, ctx, names)
        p.run_graph()
        p.sync()
        diff = R.first_difference(plan, R.read_bytes(p, names), want)
        assert diff is None, "%s, %s run_graph(): %s" % (what, call, diff)


def _stem_net(wl):
    """image 32 x 32 -> 3x3 stride-2 stem -> 1x1 conv -> global average pool -> fc (test_gpu_graphs.py's)."""
    g = wl._NetGen(11)
    g.tensor("image", 3, 32, 32, 1.0 / 127, 73.0)
    x = g.conv("stem", "image", 32, 3, 2, 1)
    x = g.conv("head", x, 64, 1, 1, 0)
    x = g.pool("pool", x, "avg", 16, 1, 0, global_pooling=True)
    return wl._finish(g, 32, g.fc("fc", x, 10))


def _plain(lite, wl, net, img):
    """name -> bytes of every variable the program writes, from a plain run of a fresh predictor lowered at 32 x 32 and resized."""
    p, plan = R.build(lite, wl, net, img.shape[0])
    try:
        p.add_feed(net["input"], img.shape, lite.PREC_FLOAT)
        p.set_input(net["input"], img)
        p.run()
        p.sync()
        names, _ = R.to_poison(plan, p.kernel_names())
        return R.read_bytes(p, names)
    finally:
        p.close()


@pytest.mark.parametrize("replay_at_b", [True, False])
def test_feed_resize_drops_the_recorded_graph(lite, wl, gpu_ctx, replay_at_b):
    """Recorded at 32 x 32, then the feed is 64 x 64 (every buffer grows: Buffer::ResetLazy frees and allocates), then 32 x 32 again
    (the recorded shapes, at the new addresses).  At every shape run() then poison then run_graph() must give the plain run of a fresh
    predictor.  replay_at_b False: no run_graph() at 64 x 64, so the graph recorded first meets its own shapes again — the shapes
    alone do not tell that it is stale; the addresses in GraphKey and the mark AddFeed leaves do."""
    net = _stem_net(wl)
    rng = np.random.default_rng(520)
    img_a = rng.uniform(-1, 1, (2, 3, 32, 32)).astype(F32)
    img_b = rng.uniform(-1, 1, (2, 3, 64, 64)).astype(F32)
    want_a, want_b = _plain(lite, wl, net, img_a), _plain(lite, wl, net, img_b)
    assert sorted(want_a) == sorted(want_b) and want_b["head"].size == 4 * want_a["head"].size
    p, plan = R.build(lite, wl, net, 2)
    try:
        p.set_input(net["input"], img_a)
        p.run()
        p.run_graph()
        p.sync()
        names = sorted(want_a)
        assert R.first_difference(plan, R.read_bytes(p, names), want_a) is None
        for img, want, replay in ((img_b, want_b, replay_at_b), (img_a, want_a, True), (img_b, want_b, True)):
            p.add_feed(net["input"], img.shape, lite.PREC_FLOAT)
            p.set_input(net["input"], img)
            p.run()
            if not replay:
                continue
            _poisoned_run_graph_equals(p, gpu_ctx, plan, names, want, "%dx%d" % img.shape[2:])
    finally:
        p.close()


def _conv_predictor(lite, x, w, bias, ws):
    """x -> io_copy -> conv 3x3 32 -> 64 [int8_out] (implicit GEMM: its padded input lives in the workspace arena) -> calib to fp32."""
    p = lite.Predictor(0)
    try:
        p.add_feed("x", x.shape, lite.PREC_INT8)
        p.add_io_copy("x", "xd", True)
        p.add_conv("conv2d", "xd", "yd", w, bias, (1, 1), (1, 1, 1, 1), (1, 1), 1, 1, 0.0, 1 / 127.0, ws, 288 / 127.0, True)
        p.add_calib("yd", "yf", 288 / 127.0, False)
        p.set_input("x", x)
        return p
    except Exception:
        p.close()
        raise


CONV_VARS = ("yd", "yf")


def _conv_case(rng, batches):
    w = rng.integers(-127, 128, (64, 32, 3, 3)).astype(np.int8)
    bias = rng.uniform(-1, 1, 64).astype(F32)
    ws = ((1 + np.arange(64) % 7) / 127.0 / 4.0).astype(F32)
    xs = [rng.integers(-127, 128, (n, 32, 28, 28)).astype(np.int8) for n in batches]
    return w, bias, ws, xs


def _conv_plain(lite, x, w, bias, ws):
    p = _conv_predictor(lite, x, w, bias, ws)
    try:
        p.run()
        p.sync()
        return R.read_bytes(p, CONV_VARS)
    finally:
        p.close()


def _on_a_fresh_thread(fn):
    """Runs fn on a new host thread (a new thread has its own HipExecState: a stream and an EMPTY workspace arena) and re-raises."""
    box = []

    def body():
        try:
            fn()
        except BaseException as e:  # noqa: BLE001
            box.append(e)
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if box:
        raise box[0]


def test_arena_replaced_by_another_predictor_drops_the_recorded_graph(lite, pkg, gpu_ctx):
    """X and Y are built on one thread and share its HipExecState.  X (batch 2) records a graph whose conv node holds the arena's
    address; Y (batch 8) needs a larger arena, so HipExecState::Workspace frees X's and allocates another.  X.run_graph() must not
    launch the recorded graph: GraphKey holds the arena's address and size, and the size only grows, so the key differs and RunGraph
    records again (a plain run first, which takes the new arena).  The thread is new, so the arena starts empty and Y's need does
    replace it whatever ran before in this process."""
    capi = pkg.capi
    need = [capi.load().plhip_conv_workspace_bytes(C.byref(capi.conv_desc(n, 32, 28, 28, 64, 3, 3, (1, 1, 1, 1)))) for n in (2, 8)]
    assert 0 < need[0] < need[1], need
    w, bias, ws, (x2, x2b, x8) = _conv_case(np.random.default_rng(521), (2, 2, 8))
    want, want_b, want8 = [_conv_plain(lite, x, w, bias, ws) for x in (x2, x2b, x8)]
    assert not np.array_equal(want["yd"], want_b["yd"])

    def body():
        X, Y = _conv_predictor(lite, x2, w, bias, ws), _conv_predictor(lite, x8, w, bias, ws)
        try:
            X.run()
            X.run_graph()
            X.sync()
            assert R.first_difference([], R.read_bytes(X, CONV_VARS), want) is None
            Y.run()   # the arena grows: freed and allocated again
            Y.sync()
            assert R.first_difference([], R.read_bytes(Y, CONV_VARS), want8) is None
            R.upload_feed(X, "x", x2b, 0)
            _poisoned_run_graph_equals(X, gpu_ctx, [], CONV_VARS, want_b, "X after Y replaced the arena")
            R.poison(Y, gpu_ctx, CONV_VARS)
            R.poison(X, gpu_ctx, CONV_VARS)
            Y.run_graph()   # Y records in the arena both now use; X replays beside it
            X.run_graph()
            Y.sync()
            assert R.first_difference([], R.read_bytes(Y, CONV_VARS), want8) is None
            assert R.first_difference([], R.read_bytes(X, CONV_VARS), want_b) is None
        finally:
            X.close()
            Y.close()
    _on_a_fresh_thread(body)


def test_two_graphs_interleaved_on_one_stream(lite, gpu_ctx):
    """The benchmark's several-predictors form in graph mode: X and Y run the same program on different inputs, share the stream and
    the workspace arena, both record; then both are poisoned and launched X, Y, X, Y with no synchronisation in between."""
    w, bias, ws, (xa, xb) = _conv_case(np.random.default_rng(522), (2, 2))
    want = [_conv_plain(lite, x, w, bias, ws) for x in (xa, xb)]
    assert not np.array_equal(want[0]["yd"], want[1]["yd"])
    X, Y = _conv_predictor(lite, xa, w, bias, ws), _conv_predictor(lite, xb, w, bias, ws)
    try:
        for p in (X, Y):
            p.run()
            p.run_graph()
            p.sync()
        for p in (X, Y):
            R.poison(p, gpu_ctx, CONV_VARS)
        for p in (X, Y, X, Y):
            p.run_graph()
        X.sync()
        for p, ref, tag in ((X, want[0], "X"), (Y, want[1], "Y")):
            diff = R.first_difference([], R.read_bytes(p, CONV_VARS), ref)
            assert diff is None, tag + ": " + diff
    finally:
        X.close()
        Y.close()


def test_run_graph_on_a_program_that_refuses_leaves_the_stream_usable(lite, gpu_ctx):
    """elementwise_mul refuses a broadcast it does not have in PrepareForRun, launching nothing.  RunGraph does one plain run before
    the capture, and that run is where this refusal is thrown: this test exercises the branch BEFORE plhip_graph_begin, not the catch
    inside the capture (no refusal that passes a plain run and throws in the recording can be made from Python without launching
    something bad).  run_graph() raises LiteError, again on a second call (no graph was kept), and a good predictor on the same thread
    and stream then runs plainly and as a graph and gives its reference bytes."""
    w, bias, ws, (x,) = _conv_case(np.random.default_rng(523), (2,))
    want = _conv_plain(lite, x, w, bias, ws)
    q = lite.Predictor(0)
    good = _conv_predictor(lite, x, w, bias, ws)
    try:
        q.add_feed("x", (2, 8, 4, 4))
        q.add_feed("y", (2, 1, 4, 4))
        q.add_io_copy("x", "xd", True)
        q.add_io_copy("y", "yd", True)
        q.add_elementwise_mul("xd", "yd", "o", 0)
        q.set_input("x", np.zeros((2, 8, 4, 4), F32))
        q.set_input("y", np.zeros((2, 1, 4, 4), F32))
        with pytest.raises(lite.LiteError, match="unsupported broadcast"):
            q.run()   # "the program must have run once before": the feeds reach the device, then the kernel refuses
        for _ in range(2):
            with pytest.raises(lite.LiteError, match="unsupported broadcast"):
                q.run_graph()
        good.run()
        good.sync()
        assert R.first_difference([], R.read_bytes(good, CONV_VARS), want) is None
        R.poison(good, gpu_ctx, CONV_VARS)
        good.run_graph()
        good.sync()
        assert R.first_difference([], R.read_bytes(good, CONV_VARS), want) is None
    finally:
        q.close()
        good.close()
