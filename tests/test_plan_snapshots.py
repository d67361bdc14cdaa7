"""GraphBuilder::Plan() against recorded plans (tests/golden/plans/, written by tools/dump_plans.py): every network, fusion switch
set, feed and batch of the tool's matrix plans line for line as it did when the fixtures were recorded.  The matrix makes every
rewrite of FuseSteps fire and not fire: conv tails (ResNet50, MobileNetV2), I / H1 / H2 (frame and image feeds), D / E / F
(MobileNetV1; D in both modes), G (MobileNetV2, MobileNetV1-192), J1 / J2 / J3 (MobileNetV3).  Exact text; no device.

A change that is meant to alter a plan rewrites the fixtures with the tool, in the same change; a refactor never does."""
import importlib
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_plans", os.path.join(ROOT, "tools", "dump_plans.py"))
dump_plans = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_plans)
ENTRIES = [e[0] for e in dump_plans.entries()]


@pytest.fixture(scope="module")
def planned(pkg):
    return dump_plans.plans(pkg)


@pytest.fixture(scope="module")
def recorded():
    return dump_plans.load_fixtures()


def test_fixtures_cover_the_matrix(recorded):
    assert sorted(recorded) == sorted(ENTRIES) and len(set(ENTRIES)) == len(ENTRIES) == 66
    limit = os.path.getsize(os.path.join(ROOT, "tests", "golden", "reference_grid.json"))
    for name in os.listdir(dump_plans.PLANS_DIR):
        assert os.path.getsize(os.path.join(dump_plans.PLANS_DIR, name)) < limit, name
    for net in ("mbv1", "mbv3_small"):  # a frame of the network's size in an interleaved format is an image feed
        for sw in ("nofuse", "default"):
            assert recorded["%s.%s.bgr_224x224.b2" % (net, sw)] == recorded["%s.%s.image_bgr.b2" % (net, sw)]


@pytest.mark.parametrize("entry", ENTRIES)
def test_plan_equals_snapshot(planned, recorded, entry):
    got, want = planned[entry], recorded[entry]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: line %d differs\n  planned : %s\n  recorded: %s" % (entry, i + 1, g, w)
    assert len(got) == len(want), "%s: %d lines planned, %d recorded; first extra line: %s" % (
        entry, len(got), len(want), (got + want)[min(len(got), len(want))])


def _dw_pw_plan(pkg, dw_strides):
    """stem 3x3 s2 -> depthwise 3x3 (512 @ 14x14, `dw_strides`) -> 1x1 512 -> 512 -> pool -> fc, through the model loader (the one
    way into the builder that takes an op's attribute lists as they come); default fusion settings, batch 2."""
    lite = importlib.import_module(pkg.__name__ + ".liteapi")
    mf = importlib.import_module(pkg.__name__ + ".modelfile")
    b = mf.SlimBuilder(7)
    x = b.feed("image", (3, 28, 28))
    x = b.conv_bn("stem", x, 3, 512, 3, 2, 1, x_abs_max=1.0)
    x = b.conv_bn("dw", x, 512, 512, 3, 1, 1, groups=512)
    x = b.conv_bn("pw", x, 512, 512, 1, 1, 0)
    x = b.pool("pool", x, "avg", 14, 1, 0, global_pooling=True)
    x = b.fc("logits", x, 512, 10, x_abs_max=2.0)
    b.fetch(x)
    (dw,) = [o for o in b.ops if o["type"] == "depthwise_conv2d"]
    dw["attrs"]["strides"] = list(dw_strides)
    p = lite.Predictor(planner=True)
    try:
        p.load_model(mf.write_container(None, b.tensors, b.ops), 2)
        return p.graph_plan()
    finally:
        p.close()


def test_depthwise_without_strides_stays_two_instructions(pkg):
    """A depthwise conv whose `strides` list is empty has no descriptor to ask the fused kernel's predicate with: fusion D leaves the
    pair alone (it used to index the empty list).  The same graph with strides {1, 1} is the pair the 14 x 14 kernel takes."""
    good, bad = _dw_pw_plan(pkg, (1, 1)), _dw_pw_plan(pkg, ())
    assert good[3].startswith("depthwise_conv2d/int8_out in=stem out=pw oscale=") and good[3].endswith(" +pw=conv2d/fp32_out via=dw"), good
    assert bad[3].startswith("depthwise_conv2d/int8_out in=stem out=dw oscale=") and "+pw=" not in bad[3], bad
    assert bad[4] == "conv2d/fp32_out in=dw out=pw", bad
    assert bad[:3] == good[:3] and bad[5:] == good[4:] and len(bad) == 9
