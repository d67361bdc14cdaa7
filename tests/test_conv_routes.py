"""The conv routes of the C ABI against recorded answers (tests/golden/conv_routes/, written by tools/dump_conv_routes.py): which
implementation a descriptor gets, its packed-weight and workspace bytes, and what the calib / image stems and the two fused
depthwise pairs say about it.  Whole lines for the workload networks' descriptors, the edge-case routes, the descriptors of
test_descriptor_helpers and invalid descriptors; per-group digests for the boundary sweep under every routing knob.  Exact text;
no device.

A change that is meant to alter a route rewrites the fixtures with the tool, in the same change; a refactor never does."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_conv_routes", os.path.join(ROOT, "tools", "dump_conv_routes.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)
IMPLS = {"conv1x1s1_gemm_int8_mfma32x32x32", "conv_3x3s2_direct_int8_mfma32x32x32", "conv_3x3s2_direct_int8_dot4",
         "conv_7x7s2_direct_int8_mfma32x32x32", "conv_patch_gemm_int8_mfma32x32x32", "conv_patch_s2_gemm_int8_mfma32x32x32",
         "conv_implicit_gemm_int8_mfma32x32x32", "conv_im2col_gemm_int8_mfma32x32x32"}


def test_fixtures_cover_every_route_and_stay_small():
    lines, sweep = dump.load_fixture("lines.txt"), dump.load_fixture("sweep.txt")
    assert 200 <= len(lines) and len(set(lines)) == len(lines)
    assert {ln.split(" | ")[1].split()[0] for ln in lines} == IMPLS | {"invalid"}
    for ln in lines:  # an invalid descriptor answers invalid / 0 / 0 and is refused by every predicate
        if " | invalid " in ln:
            assert ln.split(" | ")[1:] == ["invalid 0 0", "0 0", "0000", "00000000"], ln
    assert len(sweep) == len(dump.KNOB_SETTINGS) * 4 * 2 * 2 * 3
    seen = set()
    for ln in sweep:
        seen |= {kv.split("=")[0] for kv in ln.split()[6:-1]}
    assert seen == IMPLS | {"invalid"}
    for name in os.listdir(dump.ROUTES_DIR):
        assert os.path.getsize(os.path.join(dump.ROUTES_DIR, name)) < 256 * 1024, name


def test_lines_equal_snapshot(pkg):
    got, want = dump.full_lines(pkg), dump.load_fixture("lines.txt")
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d differs\n  library : %s\n  recorded: %s" % (i + 1, g, w)
    assert len(got) == len(want)


@pytest.mark.parametrize("setting", dump.KNOB_SETTINGS, ids=[s[0] for s in dump.KNOB_SETTINGS])
def test_sweep_equals_snapshot(pkg, setting):
    """A digest that differs names its group; `tools/dump_conv_routes.py --full DIR` on both builds shows the lines."""
    want = [ln for ln in dump.load_fixture("sweep.txt") if ln.split()[0] == setting[0]]
    got = dump.sweep_summary(setting[0], dump.sweep_groups(pkg, setting))
    assert len(got) == len(want) == 48
    for g, w in zip(got, want):
        assert g == w, "the sweep group differs\n  library : %s\n  recorded: %s" % (g, w)


GEMM_IMPLS = {"conv1x1s1_gemm_int8_mfma32x32x32", "conv_implicit_gemm_int8_mfma32x32x32", "conv_im2col_gemm_int8_mfma32x32x32"}


def test_every_gemm_route_line_has_a_launch_plan(pkg):
    """What takes_implicit used to guarantee by copying the launchers' thresholds: a descriptor the route table sends to a GEMM
    route gets a launch plan from the same function the launcher executes (csrc/gemm_plan.h), for every output kind and fused
    tail, and never the "none" outcome that run_implicit reports as unsupported.  The other routes answer no plan."""
    capi, n_gemm = pkg.capi, 0
    for ln in dump.load_fixture("lines.txt"):
        f, impl = ln.split(" | ")[0].split(), ln.split(" | ")[1].split()[0]
        if impl == "invalid":
            continue
        v = [int(x) for x in f]
        d = capi.conv_desc(*v[:7], pad=v[7:11], stride=v[11:13], dil=v[13:15], groups=v[15])
        cases = [(capi.OUT_I32, 0), (capi.OUT_I8, 0), (capi.OUT_F32, 0), (capi.OUT_F32, capi.TAIL_RESIDUAL),
                 (capi.OUT_F32, capi.TAIL_INT8_COPY | capi.TAIL_NO_F32)]
        for out, tail in cases:
            plan = capi.gemm_plan_text(d, out, tail)
            if impl in GEMM_IMPLS:
                assert plan and " family=" in plan and " family=none " not in plan, (ln, out, tail, plan)
            else:
                assert plan == "", (ln, plan)
        n_gemm += impl in GEMM_IMPLS
    assert n_gemm >= 100
