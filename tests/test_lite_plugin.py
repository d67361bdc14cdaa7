"""The C++ host side (paddle-lite_amd/lite): registry + kernel classes behind the reference's plugin interface.
CPU part: the library loads and the kHIP kernels are registered under the reference's op names / aliases.
GPU part: kernels driven like lite/tests/math/conv_int8_compute_test.cc:230-253 (KernelFactory -> SetContext ->
SetParam -> PrepareForRun -> Launch) and the whole MobileNetV1-INT8 program against the oracle graph."""
import importlib

import numpy as np
import pytest

import mbv1_oracle


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


def test_registry_has_reference_kernel_set(lite):
    L = lite.load()
    # conv2d / depthwise_conv2d x {int8_out, fp32_out}  (conv_compute.cc:216-252), fc x {int8out, fp32out}
    # (fc_compute.cc:368-380), calib x 2 (calib_compute.cc), io_copy x 2, pool2d, softmax
    assert L.pllite_registered_kernels(b"conv2d", lite.PREC_INT8, lite.LAYOUT_NCHW) == 2
    assert L.pllite_registered_kernels(b"depthwise_conv2d", lite.PREC_INT8, lite.LAYOUT_NCHW) == 2
    assert L.pllite_registered_kernels(b"fc", lite.PREC_INT8, lite.LAYOUT_NCHW) == 2
    assert L.pllite_registered_kernels(b"calib", lite.PREC_INT8, lite.LAYOUT_NCHW) == 2
    assert L.pllite_registered_kernels(b"io_copy", lite.PREC_ANY, lite.LAYOUT_ANY) == 2
    assert L.pllite_registered_kernels(b"pool2d", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1
    assert L.pllite_registered_kernels(b"pool2d", lite.PREC_INT8, lite.LAYOUT_NCHW) == 1  # product of the kHIP graph fusion
    # fp32-only on the reference's ARM target too (elementwise_compute.cc:385-412)
    assert L.pllite_registered_kernels(b"elementwise_add", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1
    assert L.pllite_registered_kernels(b"fusion_elementwise_add_activation", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1
    assert L.pllite_registered_kernels(b"elementwise_add", lite.PREC_INT8, lite.LAYOUT_NCHW) == 0
    assert L.pllite_registered_kernels(b"softmax", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 1
    assert L.pllite_registered_kernels(b"conv2d", lite.PREC_FLOAT, lite.LAYOUT_NCHW) == 0


def test_workload_matches_survey_layer_table(wl):
    m = wl.mobilenet_v1_macs()
    assert m["pointwise"] == 539492352 and m["depthwise"] == 17385984 and m["first"] == 10838016
    assert m["act_bytes"] == 10185728
    assert len(wl.mobilenet_v1_layers()) == 27


def test_predictor_without_gpu_raises(lite):
    L = lite.load()
    import ctypes
    from paddle_lite_amd import capi
    if capi.load().plhip_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(lite.LiteError):
        lite.Predictor(0)


def _single_conv(lite, plref, rng, op_type, n, cin, h, cout, k, s, pads, g, act, coef, int8_out, dil=1, algo=""):
    x = rng.integers(-127, 128, (n, cin, h, h)).astype(np.int8)
    w = rng.integers(-127, 128, (cout, cin // g, k, k)).astype(np.int8)
    bias = rng.uniform(-1, 1, cout).astype(np.float32)
    w_scale = ((1 + np.arange(cout) % 7) / 127.0 / 4.0).astype(np.float32)
    kk = (cin // g) * k * k
    in_scale, out_scale = 1 / 127.0, (kk / 127.0 if act != 2 else coef / 127.0)
    p = lite.Predictor(0)
    try:
        p.add_feed("x", x.shape, lite.PREC_INT8)
        p.add_io_copy("x", "xd", True)
        p.add_conv(op_type, "xd", "yd", w, bias, (s, s), pads, (dil, dil), g, act, coef, in_scale, w_scale, out_scale, int8_out, algo)
        p.add_io_copy("yd", "y", False)
        p.set_input("x", x)
        p.run()
        p.run()  # second launch: ReInitWhenNeeded no-op path
        y = p.get_var("y", np.int8 if int8_out else np.float32)
        names = p.kernel_names()
    finally:
        p.close()
    pads4 = pads if len(pads) == 4 else (pads[0], pads[0], pads[1], pads[1])
    if algo == "SAME":
        oh = (h + s - 1) // s
        ps = max((oh - 1) * s + k - h, 0)
        pads4 = (ps // 2, ps - ps // 2, ps // 2, ps - ps // 2)
        dil = 1
    sh = plref.shape(n, cin, h, h, cout, k, k, pads4, (s, s), (dil, dil), g)
    y_ref, _ = plref.conv2d(sh, x, w, bias, in_scale, w_scale, out_scale, act, coef, int8_out)
    return y, y_ref, names


@pytest.mark.gpu
def test_conv_kernel_classes_vs_oracle(lite, plref):
    rng = np.random.default_rng(200)
    cases = [
        ("conv2d", 2, 16, 14, 24, 1, 1, (0, 0, 0, 0), 1, 1, 0.0),          # 1x1 -> direct MFMA GEMM
        ("conv2d", 1, 8, 17, 5, 3, 1, (1, 2, 2, 1), 1, 2, 6.0),            # 3x3 s1 asymmetric pads, relu6
        ("conv2d", 2, 3, 19, 33, 3, 2, (1, 1), 1, 4, 0.25),                # 3x3 s2, 2-element paddings, leaky
        ("depthwise_conv2d", 2, 32, 15, 32, 3, 1, (1, 1, 1, 1), 32, 1, 0.0),
        ("depthwise_conv2d", 1, 5, 33, 5, 5, 2, (2, 2, 2, 2), 5, 2, 6.0),
        ("conv2d", 1, 8, 9, 6, 3, 1, (1, 1, 1, 1), 2, 0, 0.0),             # grouped
    ]
    for (op, n, cin, h, cout, k, s, pads, g, act, coef) in cases:
        for int8_out in (True, False):
            y, y_ref, names = _single_conv(lite, plref, rng, op, n, cin, h, cout, k, s, pads, g, act, coef, int8_out)
            if int8_out:
                assert np.array_equal(y, y_ref), (op, cin, cout, k, s)
            else:
                np.testing.assert_allclose(y, y_ref, rtol=1e-5, atol=1e-6)
            assert any(("int8_out" if int8_out else "fp32_out") in s_ for s_ in names)
    # padding_algorithm == "SAME" rewrites paddings in InferShape (conv_op.cc:55-81)
    y, y_ref, _ = _single_conv(lite, plref, rng, "conv2d", 1, 4, 15, 6, 3, 2, (0, 0, 0, 0), 1, 1, 0.0, True, algo="SAME")
    assert y.shape == y_ref.shape and np.array_equal(y, y_ref)


@pytest.mark.gpu
def test_feed_resize_across_an_implementation_boundary_repacks_the_weights(lite, plref):
    """The conv implementation — and with it the packed weight layout — depends on the input shape: a dense 3x3 64 -> 64
    runs on the patch kernel at W = 56 (row pitch 64) and on the implicit GEMM at W = 112; the 7x7 stride-2 stem runs on its
    direct kernel when OW % 4 == 0 and on the implicit GEMM otherwise.  A predictor whose feed is resized across such a
    boundary (AddFeed on the existing name) must repack (ConvCompute::ReInitWhenNeeded -> PackWeights) — running the new
    implementation on the old layout would return wrong numbers with no fault.  Every shape is compared with the oracle, and
    going BACK to the first shape must reproduce the first result."""
    rng = np.random.default_rng(201)
    for (cin, cout, k, s, pad, sizes, want_impls) in [
            (64, 64, 3, 1, 1, (56, 112, 56, 30), ("conv_patch", "conv_implicit_gemm", "conv_patch", "conv_patch")),
            (3, 64, 7, 2, 3, (224, 226, 224), ("conv_7x7s2_direct", "conv_implicit_gemm", "conv_7x7s2_direct"))]:
        w = rng.integers(-127, 128, (cout, cin, k, k)).astype(np.int8)
        bias = rng.uniform(-1, 1, cout).astype(np.float32)
        w_scale = ((1 + np.arange(cout) % 7) / 127.0 / 4.0).astype(np.float32)
        in_scale, out_scale = 1 / 127.0, cin * k * k / 127.0 / 4
        p = lite.Predictor(0)
        try:
            first = None
            for i, (hw, impl) in enumerate(zip(sizes, want_impls)):
                x = rng.integers(-127, 128, (2, cin, hw, hw)).astype(np.int8) if i != 2 else first[0]
                p.add_feed("x", x.shape, lite.PREC_INT8)
                if i == 0:
                    p.add_io_copy("x", "xd", True)
                    p.add_conv("conv2d", "xd", "yd", w, bias, (s, s), (pad,) * 4, (1, 1), 1, 1, 0.0, in_scale, w_scale, out_scale, True)
                    p.add_io_copy("yd", "y", False)
                p.set_input("x", x)
                p.run()
                y = p.get_var("y", np.int8)
                sh = plref.shape(2, cin, hw, hw, cout, k, k, (pad,) * 4, (s, s), (1, 1), 1)
                y_ref, _ = plref.conv2d(sh, x, w, bias, in_scale, w_scale, out_scale, 1, 0.0, True, via_gemm=True)
                assert y.shape == y_ref.shape and np.array_equal(y, y_ref), (cin, cout, k, hw, int((y != y_ref).sum()))
                name = p.time_instruction(1, 1)[2]  # the kernel the conv instruction ran (KernelBase::SetProfileRuntimeKernelInfo)
                assert name.startswith(impl), (hw, name, impl)
                if i == 0:
                    first = (x, y)
                if i == 2:
                    assert np.array_equal(y, first[1])
        finally:
            p.close()


@pytest.mark.gpu
def test_bad_weight_scale_is_fatal(lite):
    """weights scale size must equal filter number or 1 (conv_gemmlike.cc:213-215) -> LOG(FATAL)."""
    p = lite.Predictor(0)
    try:
        x = np.zeros((1, 4, 8, 8), np.int8)
        p.add_feed("x", x.shape, lite.PREC_INT8)
        p.add_io_copy("x", "xd", True)
        p.add_conv("conv2d", "xd", "yd", np.zeros((6, 4, 1, 1), np.int8), None, (1, 1), (0, 0, 0, 0), (1, 1), 1, 0, 0.0,
                   1.0, np.ones(3, np.float32), 1.0, True)
        p.set_input("x", x)
        with pytest.raises(lite.LiteError, match="weights scale size"):
            p.run()
    finally:
        p.close()


@pytest.mark.gpu
def test_mobilenet_v1_int8_program_vs_oracle_graph(lite, wl, plref):
    """Whole Appendix-D program at batch 2: every int8 activation bit-exact, fp32 tail within 1e-5."""
    W = wl.make_mobilenet_v1_weights(seed=1234)
    rng = np.random.default_rng(201)
    img = rng.uniform(-1, 1, (2, 3, 224, 224)).astype(np.float32)
    ref = mbv1_oracle.forward(plref, wl, W, img)
    p = lite.Predictor(0)
    try:
        out = wl.build_mobilenet_v1(p, W, 2)
        p.set_input("image", img)
        p.run()
        names = p.kernel_names()
        assert len(names) == 2 + 1 + 27 + 4 and sum("depthwise" in n for n in names) == 13
        for name in ["x0", "conv1", "dw2", "pw2", "dw7", "pw7", "dw14"]:
            got = p.get_var(name, np.int8)
            assert np.array_equal(got, ref[name]), name
            # synthetic scales keep the activations alive: not all-zero, not saturated
            assert 0.02 < (got != 0).mean() and (np.abs(got.astype(np.int32)) == 127).mean() < 0.2, name
        np.testing.assert_allclose(p.get_var("pw14", np.float32), ref["pw14"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(p.get_var("pool", np.float32), ref["pool"], rtol=1e-5, atol=1e-6)
        assert np.array_equal(p.get_var("pool_i8", np.int8), ref["pool_i8"])
        np.testing.assert_allclose(p.get_var("logits", np.float32), ref["logits"], rtol=1e-5, atol=1e-5)
        prob = p.get_var(out, np.float32)
        np.testing.assert_allclose(prob, ref["prob"], rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(prob.sum(-1), 1.0, rtol=1e-5)
        # second run with the feed already on the device (bench mode) gives the same answer
        p.run(skip_io_copy=True)
        assert np.array_equal(p.get_var("dw14", np.int8), ref["dw14"])
    finally:
        p.close()


@pytest.mark.gpu
def test_concurrent_predictors_reproduce_the_serial_result(lite, wl, plref):
    """bench.py's default mode: several predictors (one host thread + HIP stream each) run whole batches concurrently.
    Kernels of different predictors then share CUs, LDS and the memory pipes; every run of every predictor must still
    give exactly the bytes a lone predictor gives (int8 activations and fp32 probabilities compared bit for bit).
    Batch 32 puts the 14x14 / 7x7 layers on the same kernels as the benchmark (ring GEMM, staged depthwise)."""
    import threading
    B, P, ITERS = 32, 3, 25
    W = wl.make_mobilenet_v1_weights(seed=4321)
    img = np.random.default_rng(202).uniform(-1, 1, (B, 3, 224, 224)).astype(np.float32)
    names = ["conv1", "pw4", "dw8", "pw8", "dw14"]
    ref = {}
    p0 = lite.Predictor(0)
    try:
        out = wl.build_mobilenet_v1(p0, W, B)
        p0.set_input("image", img)
        p0.run()
        p0.sync()
        for n in names:
            ref[n] = p0.get_var(n, np.int8)
        ref[out] = p0.get_var(out, np.float32)
    finally:
        p0.close()
    errs = []
    start = threading.Barrier(P)

    def worker(i):
        try:
            p = lite.Predictor(0)  # the HIP context and its stream are per host thread (TargetWrapperHip)
            try:
                o = wl.build_mobilenet_v1(p, W, B)
                p.set_input("image", img)
                p.run()
                p.sync()
                start.wait()
                for it in range(ITERS):
                    for _ in range(3):  # a few back-to-back steps keep all three streams busy between the checks
                        p.run(skip_io_copy=True)
                    p.sync()
                    for n in names:
                        if not np.array_equal(p.get_var(n, np.int8), ref[n]):
                            errs.append("predictor %d iteration %d: %s differs" % (i, it, n))
                    if not np.array_equal(p.get_var(o, np.float32), ref[out]):
                        errs.append("predictor %d iteration %d: probabilities differ" % (i, it))
                    if errs:
                        return
            finally:
                p.close()
        except Exception as e:  # noqa: BLE001
            errs.append("predictor %d: %r" % (i, e))
            try:
                start.abort()
            except Exception:  # noqa: BLE001
                pass

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs[:5]



@pytest.mark.gpu
def test_predictors_of_one_model_share_the_packed_weights(lite, wl):
    """The serving shape of lite/api/cxx_api.h:103-137 (a predictor per thread, Clone() sharing the persistable variables):
    here the pre-packed DEVICE copy a conv / fc kernel object owns is shared per process and device, keyed on the weight
    bytes and the packing (packed_weight_cache.h).  A second predictor of the same model packs nothing, computes the same
    bytes, and the copies die with the last predictor that uses them."""
    import ctypes as C
    L = lite.load()

    def stats():
        h, m = C.c_long(), C.c_long()
        L.pllite_packed_weight_cache_stats(C.byref(h), C.byref(m))
        return h.value, m.value

    B = 2
    W = wl.make_mobilenet_v1_weights(seed=77)
    img = np.random.default_rng(203).uniform(-1, 1, (B, 3, 224, 224)).astype(np.float32)
    h0, m0 = stats()
    p1 = lite.Predictor(0)
    p2 = lite.Predictor(0)
    try:
        o1 = wl.build_mobilenet_v1(p1, W, B)
        p1.set_input("image", img)
        p1.run()
        p1.sync()
        h1, m1 = stats()
        assert m1 - m0 == 28 and h1 == h0, (h0, m0, h1, m1)  # 27 convs + fc packed once
        o2 = wl.build_mobilenet_v1(p2, W, B)
        p2.set_input("image", img)
        p2.run()
        p2.sync()
        h2, m2 = stats()
        assert m2 == m1 and h2 - h1 == 28, (h1, m1, h2, m2)  # the second predictor found all of them
        assert np.array_equal(p1.get_var(o1, np.float32), p2.get_var(o2, np.float32))
        assert np.array_equal(p1.get_var("pw8", np.int8), p2.get_var("pw8", np.int8))
    finally:
        p1.close()
        p2.close()
    p3 = lite.Predictor(0)
    try:
        wl.build_mobilenet_v1(p3, W, B)
        p3.set_input("image", img)
        p3.run()
        p3.sync()
        h3, m3 = stats()
        assert m3 - m2 == 28, (m2, m3)  # the shared copies died with p1 / p2: packed again
    finally:
        p3.close()


@pytest.mark.gpu
def test_predictor_keeps_its_stream_across_threads(lite, plref):
    """The execution state (stream + workspace) belongs to the predictor, not to the calling thread: built on one
    thread, run on another, read back on a third — same bytes (lite/backends/cuda/context.h keeps the stream in the
    context object; round 1 kept it in thread_local state and silently switched streams)."""
    import threading
    rng = np.random.default_rng(210)
    x = rng.integers(-127, 128, (4, 32, 28, 28)).astype(np.int8)
    w = rng.integers(-127, 128, (64, 32, 3, 3)).astype(np.int8)
    bias = rng.uniform(-1, 1, 64).astype(np.float32)
    ws = ((1 + np.arange(64) % 7) / 127.0 / 4.0).astype(np.float32)
    box, errs = {}, []

    def build():
        try:
            p = lite.Predictor(0)
            p.add_feed("x", x.shape, lite.PREC_INT8)
            p.add_io_copy("x", "xd", True)
            p.add_conv("conv2d", "xd", "yd", w, bias, (1, 1), (1, 1, 1, 1), (1, 1), 1, 1, 0.0, 1 / 127.0, ws, 288 / 127.0, True)
            p.add_io_copy("yd", "y", False)
            p.set_input("x", x)
            box["p"] = p
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    def run():
        try:
            for _ in range(3):
                box["p"].run()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    for fn in (build, run):
        t = threading.Thread(target=fn)
        t.start()
        t.join()
    assert not errs, errs
    try:
        y = box["p"].get_var("y", np.int8)
        sh = plref.shape(4, 32, 28, 28, 64, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 1)
        y_ref, _ = plref.conv2d(sh, x, w, bias, 1 / 127.0, ws, 288 / 127.0, 1, 0.0, True)
        assert np.array_equal(y, y_ref)
    finally:
        box["p"].close()


@pytest.mark.gpu
def test_device_timer_and_kernel_func_name(lite):
    """profile::DeviceTimer<TargetType::kHIP> (hipEvents on the context's stream, member set of timer.h:123-158) times a
    conv launch, and the kernel reports its device function through SetProfileRuntimeKernelInfo like
    conv_gemmlike.cc:384 does ("conv_im2col_gemm_int8")."""
    rng = np.random.default_rng(220)
    x = rng.integers(-127, 128, (32, 64, 56, 56)).astype(np.int8)
    w = rng.integers(-127, 128, (128, 64, 3, 3)).astype(np.int8)
    p = lite.Predictor(0)
    try:
        p.add_feed("x", x.shape, lite.PREC_INT8)
        p.add_io_copy("x", "xd", True)
        p.add_conv("conv2d", "xd", "yd", w, None, (1, 1), (1, 1, 1, 1), (1, 1), 1, 1, 0.0, 1 / 127.0, np.full(128, 1 / 127.0, np.float32),
                   576 / 127.0, True)
        p.add_calib("yd", "yf", 576 / 127.0, False)
        p.set_input("x", x)
        p.run()
        avg, mn, name = p.time_instruction(1, reps=20)
        assert name.startswith("conv_") and "gemm_int8" in name
        # 14.8 GOP: between the MFMA roof (3 us) and a generous upper bound; min <= avg; laps are real device time
        assert 0.002 < mn <= avg < 5.0
        _, _, cname = p.time_instruction(2, reps=2)
        assert cname == "int8_to_fp32_hip"
        assert p.time_instruction(0, reps=1)[2] == "io_copy_host_to_hip"
    finally:
        p.close()


@pytest.mark.gpu
def test_launch_graph_replays_the_program_bit_for_bit(lite, wl, plref, gpu_ctx):
    """HipPredictor::RunGraph: the device part of the program recorded once as a launch graph (plhip_graph_*) and replayed
    must produce exactly the bytes of the instruction-by-instruction run — also after the feed changed (the graph holds
    device addresses, not data).  Every variable the plan writes is filled with the poison byte in front of each compared
    replay, and the second image reaches the predictor through its io_copy instruction alone: what is compared is what the
    replay wrote, against the plain run of a second predictor."""
    import replay_cases as R
    net = wl.mobilenet_v1_net(seed=11)
    rng = np.random.default_rng(12)
    img = rng.uniform(-1, 1, (2, 3, 224, 224)).astype(np.float32)
    img2 = rng.uniform(-1, 1, (2, 3, 224, 224)).astype(np.float32)
    p = lite.Predictor(0)
    p2 = lite.Predictor(0)
    try:
        wl.emit_graph(p, net, 2)
        plan = p.graph_plan()
        p.graph_lower()
        p.set_input(net["input"], img)
        p.run()
        want = p.get_var(net["output"], np.float32).copy()
        names, kept = R.to_poison(plan, p.kernel_names())
        assert kept == ["image/target_trans"] and net["output"] in names and len(names) == 17
        want_all = R.read_bytes(p, names)
        p.run_graph()   # records, then launches
        R.poison(p, gpu_ctx, names)
        p.run_graph()   # replays
        assert np.array_equal(p.get_var(net["output"], np.float32), want)
        assert R.first_difference(plan, R.read_bytes(p, names), want_all) is None
        # the second image: a plain run of a second predictor is the reference; the first sees it in the replay only
        wl.emit_graph(p2, net, 2)
        p2.graph_lower()
        p2.set_input(net["input"], img2)
        p2.run()
        p2.sync()
        want2 = p2.get_var(net["output"], np.float32).copy()
        want2_all = R.read_bytes(p2, names)
        assert not np.array_equal(want, want2)
        R.upload_feed(p, net["input"], img2, R.feeds(plan)[1][0])
        R.poison(p, gpu_ctx, names)
        assert not np.array_equal(p.get_var(net["output"], np.float32), want2)
        p.run_graph()
        assert np.array_equal(p.get_var(net["output"], np.float32), want2)
        diff = R.first_difference(plan, R.read_bytes(p, names), want2_all)
        assert diff is None, diff
    finally:
        p.close()
        p2.close()
