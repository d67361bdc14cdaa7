"""-m gpu: workloads.seg_mini_net (a DeepLabV3+-shaped net: dilated convs, two interps in the decoder, interp -> arg_max as the
head) as a whole program at res 64, batch 2 and batch 3.  The programs with fusions M and N on, with both off, and with no
graph-level fusion at all are bit-identical in every fetched tensor; against interp_oracle.forward the int8 tensors are exact,
the fp32 ones within 1e-5, and the device's labels are exactly the oracle's interp + arg_max applied to the DEVICE's logits.
Against the oracle's own labels a pixel may differ only where the oracle's two largest resampled logits are closer than
2e-5 * max|logit| (twice the fp32 rule: once for each of the two logits), and at most 1 % of the pixels may be excused that way;
on the oracle 1 of 8192 pixels of the committed seed is that close (tests/test_interp_host.py checks the share on the CPU)."""
import importlib

import numpy as np
import pytest

import interp_oracle as I

pytestmark = pytest.mark.gpu
F32 = np.float32
RES = 64
# the low-resolution logits are fetched beside the labels; the int8 tensor behind the nearest interp (N's product) and the fp32 tensor
# the other interp wrote are read where they live, on the device (every program writes them)
FETCH = ("logits",)
DEVICE_VARS = ("dec_up2/precision_trans", "dec_up1")


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


@pytest.fixture(scope="module")
def segnet(wl):
    return wl.seg_mini_net(res=RES)


@pytest.fixture(scope="module")
def oracle(plref, segnet):
    """batch -> (image, name -> tensor), computed once and left unchanged."""
    out = {}
    for batch in (2, 3):
        img = np.random.default_rng(350).uniform(-1, 1, (batch, 3, RES, RES)).astype(F32)
        out[batch] = (img, I.forward(plref, segnet, img))
    return out


def _run(lite, wl, net, img, **kw):
    """Lowers and runs the net twice; returns (name -> array, plan, kernel names).  Fetching the logits does not change what M and
    N do: they are the interp's input, not the resampled tensor in front of the arg_max."""
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, img.shape[0], fetch=FETCH, **kw)
        plan = p.graph_plan()
        assert p.graph_lower() == [v + "/host" for v in FETCH] + [out]
        assert p.num_instructions() == len(plan)
        p.set_input(net["input"], img)
        p.run()
        p.run()
        got = {"label": p.get_var("label/host", np.int64), "logits": p.get_var("logits/host", F32),
               "dec_up2/precision_trans": p.get_var("dec_up2/precision_trans", np.int8), "dec_up1": p.get_var("dec_up1", F32)}
        return got, plan, p.kernel_names()
    finally:
        p.close()


@pytest.mark.parametrize("batch", [2, 3])
def test_seg_mini_net_against_the_oracle_and_between_the_programs(lite, wl, segnet, oracle, batch):
    img, ref = oracle[batch]
    on, plan_on, kernels_on = _run(lite, wl, segnet, img, fuse=True, fuse_interp_argmax=True, fuse_interp_calib=True)
    off, plan_off, _ = _run(lite, wl, segnet, img, fuse=True, fuse_interp_argmax=False, fuse_interp_calib=False)
    un, plan_un, _ = _run(lite, wl, segnet, img, fuse=False)
    heads = [l.split(" ")[0] for l in plan_on]
    assert heads.count("arg_max/interp") == 1 and heads.count("nearest_interp/int8") == 1 and heads.count("bilinear_interp/def") == 1
    assert heads.count("concat/int8") == 2 and len(plan_off) - len(plan_on) == 2
    assert not [l for l in plan_off + plan_un if l.startswith(("arg_max/interp", "nearest_interp/int8"))]
    names = "\n".join(kernels_on)
    assert "/interp -> bilinear_interp_arg_max_hip" in names and "/int8 -> nearest_interp_int8_hip" in names, names
    for v in FETCH + DEVICE_VARS + ("label",):
        assert on[v].tobytes() == off[v].tobytes(), v + ": M / N on differs from M / N off"
        assert on[v].tobytes() == un[v].tobytes(), v + ": M / N on differs from the unfused program"
    # against the oracle
    q = on["dec_up2/precision_trans"]
    assert q.shape == ref["dec_up2/precision_trans"].shape
    assert np.array_equal(q, ref["dec_up2/precision_trans"]), "%d of %d int8 values differ" % ((q != ref["dec_up2/precision_trans"]).sum(), q.size)
    for v in ("dec_up1", "logits"):
        assert on[v].shape == ref[v].shape
        np.testing.assert_allclose(on[v], ref[v], rtol=1e-5, atol=1e-5, err_msg=v)
    label = on["label"]
    assert label.shape == (batch, RES, RES) and label.dtype == np.int64 and label.min() >= 0 and label.max() < 19
    # the head itself is exact: the oracle's interp + arg_max on the logits the DEVICE made
    assert np.array_equal(label, I.arg_max(I.interp(on["logits"], (RES, RES), "bilinear", True, 1), 1))
    # against the oracle's own labels: only pixels whose two largest resampled logits are within the fp32 rule of each other
    top = np.sort(ref["logits_up"], axis=1)
    close = (top[:, -1] - top[:, -2]) < 2e-5 * float(np.abs(ref["logits"]).max())
    differ = label != ref["label"]
    print("seg_mini batch %d: %d of %d labels differ from the oracle's, %d pixels are close" % (batch, differ.sum(), differ.size, close.sum()))
    assert close.mean() <= 0.01
    assert not (differ & ~close).any(), "%d labels differ where the oracle's logits are not close" % (differ & ~close).sum()
