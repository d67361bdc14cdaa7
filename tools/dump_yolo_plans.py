#!/usr/bin/env python3
"""GraphBuilder::Plan() of the YOLOv3-shaped network (workloads.yolov3_mini_net), with graph-level fusion off, at the builder's
defaults, and with fusion P (GraphBuilder::set_fuse_yolo_head) off and on, as text fixtures under tests/golden/yolo_plans/
(tests/test_yolo_plugin_host.py compares against them line for line).  tools/dump_plans.py, tools/dump_concat_plans.py,
tools/dump_interp_plans.py and tools/dump_detection_plans.py keep their own matrices.

The fixtures record what the planner decided at the commit they were written from.  Rewrite them
(`python tools/dump_yolo_plans.py`) only in a change that is meant to alter a plan, and review the diff.  One file per entry,
<network>.<switch set>.b<batch>.txt."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS_DIR = os.path.join(ROOT, "tests", "golden", "yolo_plans")

NETS = [
    ("yolov3_mini", lambda wl: wl.yolov3_mini_net()),
]
# keyword arguments of workloads.emit_graph; a switch that is absent keeps the builder's default
SWITCHES = [
    ("nofuse", dict(fuse=False)),
    ("default", dict(fuse=True)),
    ("p_off", dict(fuse=True, fuse_yolo_head=False)),
    ("p_on", dict(fuse=True, fuse_yolo_head=True)),
]
BATCH = 2


def entries():
    """[(name, network, batch, emit_graph keywords)]"""
    return [("%s.%s.b%d" % (net, sw, BATCH), net, BATCH, dict(kw)) for net, _ in NETS for sw, kw in SWITCHES]


def plans(pkg):
    """{entry name: plan lines} of the whole matrix from the planner of `pkg` (the imported paddle_lite_amd package)."""
    lite = importlib.import_module(pkg.__name__ + ".liteapi")
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    nets = {name: make(wl) for name, make in NETS}
    out = {}
    for name, net, batch, kw in entries():
        p = lite.Predictor(planner=True)
        try:
            wl.emit_graph(p, nets[net], batch, **kw)
            out[name] = p.graph_plan()
        finally:
            p.close()
    return out


def load_fixtures():
    """{entry name: plan lines} as recorded under tests/golden/yolo_plans/."""
    out = {}
    for name, _, _, _ in entries():
        with open(os.path.join(PLANS_DIR, name + ".txt")) as f:
            out[name] = f.read().splitlines()
    return out


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    got = plans(ge.import_package())
    os.makedirs(PLANS_DIR, exist_ok=True)
    for name, lines in got.items():
        with open(os.path.join(PLANS_DIR, name + ".txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    print("%d plans -> %s" % (len(got), PLANS_DIR))


if __name__ == "__main__":
    main()
