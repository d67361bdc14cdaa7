#!/usr/bin/env python3
"""What the C ABI answers about a conv descriptor without a device, as text fixtures under tests/golden/conv_routes/
(tests/test_conv_routes.py recomputes them from the library and compares).

A line is the descriptor and every host-only answer about it:

  n cin h w cout kh kw pt pb pl pr sh sw dh dw groups m | impl packed workspace | calib image | dwpw | dwconv

impl / packed / workspace: plhip_conv_impl_name, plhip_conv_packed_weight_bytes, plhip_conv_workspace_bytes; calib / image:
plhip_conv2d_calib_supported, plhip_conv2d_image_supported (an image of the descriptor's n, h, w: GRAY for cin 1, BGR for cin 3,
BGRA otherwise); dwpw: plhip_dwpw_fused_supported(d, m, out) for out = 0..3; dwconv: plhip_dw_conv1x1_fused_supported(d, m, out,
has_tail) for out = 0..3, has_tail 0 then 1.  m is the output channels of the 1x1 conv behind a depthwise conv.

lines.txt holds whole lines (default knobs): the conv / depthwise descriptors of the five workload networks at batch 1, 2 and
128, the shapes of tests/edge_cases.ROUTES, the descriptors of test_descriptor_helpers and a few invalid ones.  sweep.txt holds
the boundary sweep (SWEEP, batch 2, m = cout) under each knob setting of KNOB_SETTINGS, one line per (knob setting, k, stride,
dilation, groups class): the count per impl name and a sha256 over the group's whole lines.  `--full DIR` writes those whole
lines, one file per knob setting, to diff two builds when a digest differs.

The fixtures record what the library decided at the commit they were written from; a refactor of the routing must leave them
alone.  Rewrite them (`python tools/dump_conv_routes.py`) only in a change that is meant to alter a route, and review the diff."""
import argparse
import ctypes
import hashlib
import importlib
import importlib.util
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES_DIR = os.path.join(ROOT, "tests", "golden", "conv_routes")

NETS = [
    ("mbv1", lambda wl: wl.mobilenet_v1_net()),
    ("mbv2", lambda wl: wl.mobilenet_v2_net()),
    ("mbv3_large", lambda wl: wl.mobilenet_v3_net("large")),
    ("mbv3_small", lambda wl: wl.mobilenet_v3_net("small")),
    ("resnet50", lambda wl: wl.resnet50_net()),
]
BATCHES = (1, 2, 128)
# (n, cin, h, w, cout, kh, kw, pads, stride, dil, groups), as tests/edge_cases.ROUTES spells a shape
HELPER_DESCS = [
    (32, 64, 56, 56, 128, 3, 3, (1,) * 4, 1, 1, 1), (32, 48, 56, 56, 128, 3, 3, (1,) * 4, 1, 1, 1),
    (32, 64, 56, 56, 128, 3, 3, (1,) * 4, 2, 1, 1), (32, 48, 56, 56, 128, 3, 3, (1,) * 4, 2, 1, 1),
    (32, 64, 56, 56, 64, 3, 3, (1,) * 4, 2, 1, 1), (256, 3, 224, 224, 64, 7, 7, (3,) * 4, 2, 1, 1),
    (2, 4, 224, 224, 64, 7, 7, (3,) * 4, 2, 1, 1), (2, 3, 224, 226, 64, 7, 7, (3,) * 4, 2, 1, 1),
    (32, 64, 56, 56, 128, 3, 3, (2,) * 4, 1, 2, 1), (128, 512, 14, 14, 512, 1, 1, (0,) * 4, 1, 1, 1),
]
INVALID_DESCS = [
    (1, 6, 8, 8, 8, 3, 3, (0,) * 4, 1, 1, 4),        # cin % groups
    (1, 8, 8, 8, 6, 3, 3, (0,) * 4, 1, 1, 4),        # cout % groups
    (0, 8, 8, 8, 8, 3, 3, (1,) * 4, 1, 1, 1),        # no image
    (1, 8, 8, 8, 8, 3, 3, (1,) * 4, 0, 1, 1),        # stride 0
    (1, 8, 8, 8, 8, 3, 3, (1,) * 4, 1, 0, 1),        # dilation 0
    (1, 8, 8, 8, 8, 3, 3, (1, 1, -1, 1), 1, 1, 1),   # negative padding
    (1, 8, 2, 2, 8, 5, 5, (0,) * 4, 1, 1, 1),        # no output
    (1, 8, 8, 8, 8, 0, 3, (1,) * 4, 1, 1, 1),        # empty filter
    (1, 8, 8, 8, 8, 3, 3, (1,) * 4, 1, 1, 0),        # groups 0
]
SWEEP = dict(cin=(3, 4, 16, 32, 48, 64, 96, 128), cout=(8, 32, 33, 64, 65, 96, 128, 129, 256), hw=(7, 8, 14, 15, 16, 28, 56, 57),
             k=(1, 3, 5, 7), stride=(1, 2), pads=(0, 1, "k//2", (0, 1, 0, 1), (1, 0, 1, 0)), dil=(1, 2), groups=(1, 2, "cin"))
KNOB_SETTINGS = [("default", None), ("IMPLICIT_GEMM=0", "IMPLICIT_GEMM"), ("GEMM_TR=0", "GEMM_TR"), ("CONV_PATCH=0", "CONV_PATCH"),
                 ("CONV_PATCH_S2=0", "CONV_PATCH_S2"), ("STEM7=0", "STEM7")]
KNOB_DEFAULT = 1  # what the library reads each of these knobs as when nobody set it
IMG_BGRA, IMG_BGR, IMG_GRAY = 1, 3, 4


def _pads(p, k):
    p = k // 2 if p == "k//2" else p
    return (p,) * 4 if isinstance(p, int) else tuple(p)


class Asker:
    """The eight host-only calls behind one method: line(shape, m) -> the fixture line of that descriptor."""

    def __init__(self, pkg):
        self.capi = pkg.capi
        self.lib = pkg.capi.load()
        self.d = pkg.capi.conv_desc(1, 1, 1, 1, 1, 1, 1, act=pkg.capi.ACT_RELU)  # one descriptor, refilled per line
        self.img = pkg.capi.image_desc(1, 1, 1, IMG_BGR, (0.0,) * 3, (1.0,) * 3)

    def line(self, shape, m):
        n, cin, h, w, cout, kh, kw, pads, stride, dil, groups = shape
        L, d, img = self.lib, self.d, self.img
        d.n, d.cin, d.h, d.w, d.cout, d.kh, d.kw, d.groups = n, cin, h, w, cout, kh, kw, groups
        d.pad[:] = pads
        d.stride[:] = (stride, stride)
        d.dil[:] = (dil, dil)
        img.n, img.h, img.w, img.format = n, h, w, IMG_GRAY if cin == 1 else IMG_BGR if cin == 3 else IMG_BGRA
        r = ctypes.byref(d)
        dwpw = "".join(str(L.plhip_dwpw_fused_supported(r, m, out)) for out in range(4))
        dwconv = "".join(str(L.plhip_dw_conv1x1_fused_supported(r, m, out, t)) for out in range(4) for t in (0, 1))
        return "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | %s %d %d | %d %d | %s | %s" % (
            n, cin, h, w, cout, kh, kw, pads[0], pads[1], pads[2], pads[3], stride, stride, dil, dil, groups, m,
            L.plhip_conv_impl_name(r).decode(), L.plhip_conv_packed_weight_bytes(r), L.plhip_conv_workspace_bytes(r),
            L.plhip_conv2d_calib_supported(r), L.plhip_conv2d_image_supported(r, ctypes.byref(img)), dwpw, dwconv)

    def set_knob(self, key, value):
        assert self.lib.plhip_debug_set(key.encode(), value) == 0, key


def net_shapes(net, batch):
    """[(shape, m)] of a network's conv / depthwise ops; m = the output channels of the 1x1 conv that reads a depthwise conv."""
    shapes = dict(net["shapes"], **{net["input"]: net["input_shape"]})
    out = []
    for o in net["ops"]:
        if o["op"] not in ("conv2d", "depthwise_conv2d"):
            continue
        cin, h, w = shapes[o["src"]]
        cout, _, k, _ = o["w"].shape
        readers = [r for r in net["ops"] if r["op"] == "conv2d" and r["src"] == o["name"] and r["w"].shape[2] == 1]
        m = readers[0]["w"].shape[0] if o["op"] == "depthwise_conv2d" and readers else cout
        out.append(((batch, cin, h, w, cout, k, k, (o["pad"],) * 4, o["stride"], 1, o["groups"]), m))
    return out


def edge_routes():
    spec = importlib.util.spec_from_file_location("edge_cases", os.path.join(ROOT, "tests", "edge_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [(r["shape"], r["m"] or r["shape"][4]) for r in mod.ROUTES]


def full_lines(pkg):
    """The lines of lines.txt: every distinct (descriptor, m), in the order of the docstring."""
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    todo = []
    for _, make in NETS:
        net = make(wl)
        for batch in BATCHES:
            todo += net_shapes(net, batch)
    todo += edge_routes()
    todo += [(s, s[4]) for s in HELPER_DESCS + INVALID_DESCS]
    ask, seen, out = Asker(pkg), set(), []
    for shape, m in todo:
        if (shape, m) not in seen:
            seen.add((shape, m))
            out.append(ask.line(shape, m))
    return out


def sweep_groups(pkg, setting):
    """{(k, stride, dil, groups class): [lines]} of the boundary sweep under one entry of KNOB_SETTINGS; the knob is put back."""
    name, knob = setting
    ask, out = Asker(pkg), {}
    if knob:
        ask.set_knob(knob, 0)
    try:
        for k, stride, dil, gc in itertools.product(SWEEP["k"], SWEEP["stride"], SWEEP["dil"], SWEEP["groups"]):
            lines = out.setdefault((k, stride, dil, gc), [])
            pads = list(dict.fromkeys(_pads(p, k) for p in SWEEP["pads"]))
            for cin, cout, hw, pad in itertools.product(SWEEP["cin"], SWEEP["cout"], SWEEP["hw"], pads):
                lines.append(ask.line((2, cin, hw, hw, cout, k, k, pad, stride, dil, cin if gc == "cin" else gc), cout))
    finally:
        if knob:
            ask.set_knob(knob, KNOB_DEFAULT)
    return out


def sweep_summary(name, groups):
    """The lines of sweep.txt for one knob setting."""
    out = []
    for (k, stride, dil, gc), lines in groups.items():
        count = {}
        for ln in lines:
            impl = ln.split(" | ")[1].split()[0]
            count[impl] = count.get(impl, 0) + 1
        out.append("%s k=%d s=%d d=%d g=%s n=%d %s sha256=%s" % (
            name, k, stride, dil, gc, len(lines), " ".join("%s=%d" % kv for kv in sorted(count.items())),
            hashlib.sha256(("\n".join(lines) + "\n").encode()).hexdigest()))
    return out


def load_fixture(fname):
    with open(os.path.join(ROUTES_DIR, fname)) as f:
        return f.read().splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--full", metavar="DIR", help="also write the sweep's whole lines, one file per knob setting, to DIR")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.import_package()
    os.makedirs(ROUTES_DIR, exist_ok=True)
    lines = full_lines(pkg)
    with open(os.path.join(ROUTES_DIR, "lines.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    summary = []
    for setting in KNOB_SETTINGS:
        groups = sweep_groups(pkg, setting)
        summary += sweep_summary(setting[0], groups)
        if args.full:
            os.makedirs(args.full, exist_ok=True)
            with open(os.path.join(args.full, setting[0].replace("=", "_") + ".txt"), "w") as f:
                for g in groups.values():
                    f.write("\n".join(g) + "\n")
    with open(os.path.join(ROUTES_DIR, "sweep.txt"), "w") as f:
        f.write("\n".join(summary) + "\n")
    print("%d lines, %d sweep groups -> %s" % (len(lines), len(summary), ROUTES_DIR))


if __name__ == "__main__":
    main()
