#!/usr/bin/env python3
"""Predictor.kernel_names() of a fixed matrix of lowered programs after one run on the device, as text fixtures under
tests/golden/kernel_names/ (tests/test_gpu_kernel_names.py compares against them line for line).  Needs a GPU: a kernel
object names what it launches once it has seen its input's shape.

The fixtures record what the kernel objects named at the commit they were written from; a refactor of the kernel classes
must leave them alone.  Rewrite them (`python tools/dump_kernel_names.py [--out DIR]`) only in a change that is meant to alter a
name or a route, and review the diff.

An entry's name is <network>.<switch set>.<feed>.b<batch>, as in tools/dump_plans.py, whose networks and switch sets these are."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES_DIR = os.path.join(ROOT, "tests", "golden", "kernel_names")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dump_plans  # noqa: E402

BATCH = 2
MATRIX = [("mbv1", ("default", "dwconv", "dwpw_all")), ("mbv2", ("default", "dwconv", "dwpw_all")), ("mbv3_small", ("default", "all")),
          ("resnet50", ("default",)), ("two_stem", ("default",))]


def entries():
    """[(name, network, feed, emit_graph keywords)]"""
    sw = dict(dump_plans.SWITCHES)
    out = [("%s.%s.tensor.b%d" % (net, s, BATCH), net, "tensor", dict(sw[s])) for net, sws in MATRIX for s in sws]
    out.append(("mbv1.default.image_bgr.b%d" % BATCH, "mbv1", "image_bgr", dict(sw["default"], **dict(dump_plans.FEEDS)["image_bgr"])))
    return out


def kernel_names(pkg, entry):
    """The kernel names of one entry's program, lowered and run once on device 0 by `pkg` (the imported paddle_lite_amd package)."""
    lite = importlib.import_module(pkg.__name__ + ".liteapi")
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    _, net_name, feed, kw = [e for e in entries() if e[0] == entry][0]
    net = dict(dump_plans.NETS + dump_plans.EDGE_NETS)[net_name](wl)
    c, h, w = net["input_shape"]
    rng = np.random.default_rng(5)
    if feed == "tensor":
        x = rng.uniform(-1, 1, (BATCH, c, h, w)).astype(np.float32)
    else:
        x = rng.integers(0, 256, (BATCH, h, w, 3)).astype(np.uint8)
    p = lite.Predictor(0)
    try:
        wl.emit_graph(p, net, BATCH, **kw)
        p.graph_lower()
        p.set_input(net["input"], x)
        p.run()
        return p.kernel_names()
    finally:
        p.close()


def load_fixture(entry):
    with open(os.path.join(NAMES_DIR, entry + ".txt")) as f:
        return f.read().splitlines()


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.import_package()
    out_dir = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else NAMES_DIR
    os.makedirs(out_dir, exist_ok=True)
    for name, _, _, _ in entries():
        with open(os.path.join(out_dir, name + ".txt"), "w") as f:
            f.write("\n".join(kernel_names(pkg, name)) + "\n")
    print("%d entries -> %s" % (len(entries()), out_dir))


if __name__ == "__main__":
    main()
