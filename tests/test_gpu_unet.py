"""-m gpu: workloads.unet_mini_net (two encoder stages, a bottleneck, two decoder stages conv2d_transpose -> concat -> conv, a 1x1
classifier and arg_max) as a whole program at res 64, batch 2.  The fused program (the builder's defaults: fusion L takes both
concats) and the unfused one are bit-identical in every fetched and device-read tensor; against deconv_oracle.forward the int8
tensors are exact and the fp32 ones within 1e-5; the labels equal the oracle's except where its two largest logits are within
1e-5 of each other, and the count of such pixels is 0 for the committed seed (tests/test_deconv_host.py checks that on the CPU).
One replay through run_graph() into poisoned variables gives the bytes run() gave."""
import importlib

import numpy as np
import pytest

import deconv_oracle as D
import replay_cases as R

pytestmark = pytest.mark.gpu
F32 = np.float32
RES, BATCH = 64, 2
FETCH = ("logits",)
# read where they live, on the device; every program writes them: the transposed convs' fp32 outputs, the int8 tensors behind the
# concats (fusion L's product in the fused program, a calib's in the unfused one) and an int8 conv output
DEVICE_VARS = (("dec2_up", F32), ("dec1_up", F32), ("dec2_concat/precision_trans", np.int8), ("dec1_concat/precision_trans", np.int8),
               ("bottleneck", np.int8), ("dec1_conv", np.int8))


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


@pytest.fixture(scope="module")
def unet(wl):
    return wl.unet_mini_net(res=RES)


@pytest.fixture(scope="module")
def oracle(plref, unet):
    """(image, name -> tensor), computed once and left unchanged."""
    img = np.random.default_rng(350).uniform(-1, 1, (BATCH, 3, RES, RES)).astype(F32)
    return img, D.forward(plref, unet, img)


def _run(lite, wl, net, img, replay=False, ctx=None, **kw):
    """Lowers and runs the net twice; returns (name -> array, plan, kernel names)."""
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, img.shape[0], fetch=FETCH, **kw)
        plan = p.graph_plan()
        assert p.graph_lower() == [v + "/host" for v in FETCH] + [out]
        assert p.num_instructions() == len(plan)
        p.set_input(net["input"], img)
        p.run()
        p.run()

        def read():
            got = {"label": p.get_var("label/host", np.int64), "logits": p.get_var("logits/host", F32)}
            got.update({v: p.get_var(v, t) for v, t in DEVICE_VARS})
            return got
        got = read()
        if replay:
            names, kept = R.to_poison(plan, p.kernel_names())
            assert kept == ["image/target_trans"] and {"label", "logits"} | {v for v, _ in DEVICE_VARS} <= set(names), (kept, names)
            before = R.read_bytes(p, names)
            p.run_graph()  # records, then launches
            R.poison(p, ctx, names)  # every variable the plan writes: the replay has to write them all
            p.run_graph()  # replays
            p.sync()
            again = {v: p.get_var(v, t) for v, t in DEVICE_VARS + (("label", np.int64), ("logits", F32))}
            for v in again:
                assert again[v].tobytes() == got[v].tobytes(), v + ": the replayed graph differs from run()"
            diff = R.first_difference(plan, R.read_bytes(p, names), before)
            assert diff is None, "the replayed graph differs from run(): " + diff
        return got, plan, p.kernel_names()
    finally:
        p.close()


def test_unet_mini_net_against_the_oracle_and_between_the_programs(lite, wl, unet, oracle, gpu_ctx):
    img, ref = oracle
    on, plan_on, kernels_on = _run(lite, wl, unet, img, replay=True, ctx=gpu_ctx, fuse=True)
    un, plan_un, _ = _run(lite, wl, unet, img, fuse=False)
    heads = [l.split(" ")[0] for l in plan_on]
    assert heads.count("conv2d_transpose/fp32_out") == 2 and heads.count("concat/int8") == 2 and len(plan_un) - len(plan_on) == 2
    names = "\n".join(kernels_on)
    assert names.count("deconv_phase_int8_mfma32x32x32") == 2, names   # both transposed convs run the MFMA phase route
    for v in [v for v, _ in DEVICE_VARS] + ["logits", "label"]:
        assert on[v].tobytes() == un[v].tobytes(), v + ": the fused program differs from the unfused one"
    # against the oracle
    for v, t in DEVICE_VARS:
        assert on[v].shape == ref[v].shape and on[v].dtype == ref[v].dtype, v
        if t == np.int8:
            assert np.array_equal(on[v], ref[v]), "%s: %d of %d int8 values differ" % (v, (on[v] != ref[v]).sum(), on[v].size)
        else:
            np.testing.assert_allclose(on[v], ref[v], rtol=1e-5, atol=1e-5, err_msg=v)
    np.testing.assert_allclose(on["logits"], ref["logits"], rtol=1e-5, atol=1e-5, err_msg="logits")
    label = on["label"]
    assert label.shape == (BATCH, RES, RES) and label.dtype == np.int64 and label.min() >= 0 and label.max() < 4
    top = np.sort(ref["logits"], axis=1)
    close = (top[:, -1] - top[:, -2]) < 1e-5
    differ = label != ref["label"]
    print("unet_mini batch %d: %d of %d labels differ from the oracle's, %d pixels have their two largest logits within 1e-5" % (
        BATCH, differ.sum(), differ.size, close.sum()))
    assert close.sum() == 0
    assert not (differ & ~close).any(), "%d labels differ where the oracle's logits are not close" % (differ & ~close).sum()
