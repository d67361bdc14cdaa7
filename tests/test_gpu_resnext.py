"""-m gpu: the ResNeXt50-32x4d INT8 program (workloads.resnext50_net) against the oracle graph, every variable of the lowered
program, unfused and with the default fusions; its 16 grouped 3x3 convs run the grouped route (conv_grouped_i8.hip).

Resolution 96 at batch 2: the planes are 24 / 12 / 6 / 3, so the last stage runs the stride-2 grouped conv onto a 3x3 plane and
the stride-1 one on it.  The plans and kernel names of this program are recorded under tests/golden/resnext/
(`python tests/test_gpu_resnext.py` rewrites them; the kernel names need the device)."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "resnext")
GROUPED = "conv_grouped3x3_int8_mfma32x32x32"
RES, BATCH = 96, 2
SWITCHES = (("nofuse", False), ("default", True))


def _fixture(name):
    with open(os.path.join(FIXTURES, name)) as f:
        return f.read().splitlines()


def _image():
    return np.random.default_rng(350).uniform(-1, 1, (BATCH, 3, RES, RES)).astype(np.float32)


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module(pkg.__name__ + ".liteapi")


@pytest.fixture(scope="module")
def net(pkg):
    return importlib.import_module(pkg.__name__ + ".workloads").resnext50_net(res=RES)


@pytest.fixture(scope="module")
def ref(net, plref):
    from oracle import graph_oracle
    out = graph_oracle.forward(plref, net, _image())
    for v in out.values():
        v.setflags(write=False)
    return out


def _lowered(pkg, lite, net, fuse):
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    p = lite.Predictor(0)
    try:
        out = wl.emit_graph(p, net, BATCH, fuse=fuse)
        assert p.graph_lower() == [out]
        p.set_input(net["input"], _image())
        p.run()
        p.run(skip_io_copy=False)  # second launch: ReInitWhenNeeded no-op paths
        return p, out
    except Exception:
        p.close()
        raise


def _live(plan):
    """The variables a plan still produces (a fused tail may drop the fp32 tensor and adds the calib copy)."""
    live = set()
    for l in plan:
        o = l.split(" out=")[1].split(" ")[0]
        if not l.endswith("-f32") and " -f32" not in l:
            live.add(o)
        if "+calib=" in l:
            live.add(l.split("+calib=")[1].split(" ")[0])
    return live


@pytest.mark.parametrize("switch,fuse", SWITCHES, ids=[s for s, _ in SWITCHES])
def test_resnext50_int8_program_vs_oracle_graph(pkg, lite, net, ref, switch, fuse):
    p, out = _lowered(pkg, lite, net, fuse)
    try:
        plan, names = p.graph_plan(), p.kernel_names()
        assert sum(GROUPED in n for n in names) == 16, [n for n in names if "conv" in n]
        assert plan == _fixture("plan.%s.b%d.txt" % (switch, BATCH))
        assert names == _fixture("kernel_names.%s.b%d.txt" % (switch, BATCH))
        live = _live(plan)
        n_i8 = n_f32 = 0
        for name, want in ref.items():
            if name not in live:
                continue
            got = p.get_var(name, want.dtype)
            assert got.shape == want.shape, name
            if want.dtype == np.int8:
                assert np.array_equal(got, want), "%s: %d of %d int8 values differ" % (name, (got != want).sum(), want.size)
                n_i8 += 1
            else:
                np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5, err_msg=name)
                n_f32 += 1
        # 18 calib copies + 32 int8-output convs (16 of them grouped); unfused, every fp32 tensor of the oracle is there too
        assert n_i8 >= 49 and (fuse or (n_i8 == 18 + 32 and n_i8 + n_f32 == len(ref)))
        np.testing.assert_allclose(p.get_var(out, np.float32), ref["prob"], rtol=1e-4, atol=1e-7)
        for name in ["res2a/precision_trans", "res3d_branch2b", "res5c_branch2a"]:
            got = p.get_var(name, np.int8)
            assert 0.02 < (got != 0).mean() and (np.abs(got.astype(np.int32)) == 127).mean() < 0.2, name
    finally:
        p.close()


def _write_fixtures():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.import_package()
    lite_ = importlib.import_module(pkg.__name__ + ".liteapi")
    net_ = importlib.import_module(pkg.__name__ + ".workloads").resnext50_net(res=RES)
    out_dir = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else FIXTURES
    os.makedirs(out_dir, exist_ok=True)
    for switch, fuse in SWITCHES:
        p, _ = _lowered(pkg, lite_, net_, fuse)
        try:
            for kind, lines in (("plan", p.graph_plan()), ("kernel_names", p.kernel_names())):
                with open(os.path.join(out_dir, "%s.%s.b%d.txt" % (kind, switch, BATCH)), "w") as f:
                    f.write("\n".join(lines) + "\n")
        finally:
            p.close()


if __name__ == "__main__":
    _write_fixtures()
