#!/usr/bin/env python3
"""GraphBuilder::Plan() of a fixed matrix of networks, fusion switches, feeds and batches, as text fixtures under
tests/golden/plans/ (tests/test_plan_snapshots.py compares against them line for line).

The fixtures record what the planner decided at the commit they were written from; a refactor of the planner must leave them
alone.  Rewrite them (`python tools/dump_plans.py`) only in a change that is meant to alter a plan, and review the diff.

Layout: index.txt holds one "<entry> <file>" line per entry of the matrix; entries whose plans are identical share one file,
named after the first of them.  An entry's name is <network>.<switch set>.<feed>.b<batch>."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS_DIR = os.path.join(ROOT, "tests", "golden", "plans")


def two_stem_net(wl):
    """Two 3x3 stride-2 stems read the image through ONE calib (two readers: F must leave it alone), and the 1x1 conv behind the
    depthwise conv adds a tensor that is made between the two (G must leave the pair alone: the residual does not exist yet where
    the depthwise conv runs)."""
    g = wl._NetGen(7)
    g.tensor("image", 3, 32, 32, 1.0 / 127, 73.0)
    a = g.conv("stem_a", "image", 32, 3, 2, 1)
    b = g.conv("stem_b", "image", 32, 3, 2, 1)
    d = g.conv("dw", a, 32, 3, 1, 1, groups=32)
    side = g.conv("side", b, 32, 1, 1, 0, act=0)
    x = g.add("sum", side, g.conv("pw", d, 32, 1, 1, 0, act=0))
    x = g.conv("head", x, 64, 1, 1, 0)
    x = g.pool("pool", x, "avg", 16, 1, 0, global_pooling=True)
    return wl._finish(g, 32, g.fc("fc", x, 10))


NETS = [
    ("mbv1", lambda wl: wl.mobilenet_v1_net()),
    ("mbv1_192", lambda wl: wl.mobilenet_v1_net(res=192)),
    ("mbv2", lambda wl: wl.mobilenet_v2_net()),
    ("mbv3_large", lambda wl: wl.mobilenet_v3_net("large")),
    ("mbv3_small", lambda wl: wl.mobilenet_v3_net("small")),
    ("resnet50", lambda wl: wl.resnet50_net()),
]
EDGE_NETS = [("two_stem", two_stem_net)]  # guards no published network exercises: default switches and fusion G only
# keyword arguments of workloads.emit_graph; a switch that is absent keeps the builder's default
SWITCHES = [
    ("nofuse", dict(fuse=False)),
    ("dwpw_off", dict(fuse=True, fuse_dwpw=False)),
    ("default", dict(fuse=True)),
    ("dwpw_all", dict(fuse=True, fuse_dwpw=True)),
    ("dwconv", dict(fuse=True, fuse_dwconv=True)),
    ("hard_act", dict(fuse=True, fuse_hard_act=True)),
    ("all", dict(fuse=True, fuse_dwpw=True, fuse_dwconv=True, fuse_hard_act=True)),
]
BGR, NV21, NV12 = 3, 11, 12  # liteapi.IMG_*
MEANS = (120.0, 127.5, 135.0)
SCALES = (1 / 127.5 * 1.03, 1 / 127.5, 1 / 127.5 * 0.97)


def _frame(h, w, fmt):
    return dict(frame=dict(h=h, w=w, format=fmt, means=MEANS, scales=SCALES))


FEEDS = [
    ("image_bgr", dict(image=dict(format=BGR, means=MEANS, scales=SCALES))),
    ("nv12_480x640", _frame(480, 640, NV12)),
    ("bgr_480x640", _frame(480, 640, BGR)),
    ("nv21_224x224", _frame(224, 224, NV21)),  # convert only
    ("bgr_224x224", _frame(224, 224, BGR)),    # an image feed under another name
]


def entries():
    """[(name, network, batch, emit_graph keywords)]"""
    out = []
    for net, _ in NETS:
        for sw, kw in SWITCHES:
            out.append(("%s.%s.tensor.b2" % (net, sw), net, 2, dict(kw)))
    for net in ("mbv1", "mbv3_small"):
        for sw in ("nofuse", "default"):
            for feed, fkw in FEEDS:
                out.append(("%s.%s.%s.b2" % (net, sw, feed), net, 2, dict(dict(SWITCHES)[sw], **fkw)))
    for net, _ in EDGE_NETS:
        for sw in ("default", "dwconv"):
            out.append(("%s.%s.tensor.b2" % (net, sw), net, 2, dict(dict(SWITCHES)[sw])))
    for batch in (1, 128):
        out.append(("mbv1.default.tensor.b%d" % batch, "mbv1", batch, dict(fuse=True)))
    return out


def plans(pkg):
    """{entry name: plan lines} of the whole matrix from the planner of `pkg` (the imported paddle_lite_amd package)."""
    lite = importlib.import_module(pkg.__name__ + ".liteapi")
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    nets = {name: make(wl) for name, make in NETS + EDGE_NETS}
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
    """{entry name: plan lines} as recorded under tests/golden/plans/."""
    out, files = {}, {}
    with open(os.path.join(PLANS_DIR, "index.txt")) as f:
        for line in f:
            name, fname = line.split()
            if fname not in files:
                with open(os.path.join(PLANS_DIR, fname)) as g:
                    files[fname] = g.read().splitlines()
            out[name] = files[fname]
    return out


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    got = plans(ge.import_package())
    os.makedirs(PLANS_DIR, exist_ok=True)
    by_text, index = {}, []
    for name, _, _, _ in entries():
        text = "\n".join(got[name]) + "\n"
        if text not in by_text:
            by_text[text] = name + ".txt"
            with open(os.path.join(PLANS_DIR, by_text[text]), "w") as f:
                f.write(text)
        index.append("%s %s\n" % (name, by_text[text]))
    with open(os.path.join(PLANS_DIR, "index.txt"), "w") as f:
        f.writelines(index)
    print("%d entries, %d distinct plans -> %s" % (len(index), len(by_text), PLANS_DIR))


if __name__ == "__main__":
    main()
