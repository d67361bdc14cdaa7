"""Fusion G measurements: depthwise 3x3 [int8_out] -> 1x1 conv with its tail in one launch.

  python tools/dwconv_bench.py [--out profiles/dwconv_g.json] [--batches 1024,128] [--reps 20] [--steps 20] [--inflight 4]

1. Per block: each of MobileNetV2-224's 17 (depthwise, project) pairs with its real tail, fused
   (plhip_dw_conv1x1_fused_int8) against the two launches it replaces (plhip_depthwise_conv_int8 + plhip_conv2d_int8_fused /
   plhip_conv2d_int8), HIP events after warm-up, median of `reps`; the algorithmic bytes of both forms and their fraction of
   8 TB/s.
2. Whole program: BASELINE config C5's MobileNetV2 graph at batch 1024 with G off and G on in the same process, alternated,
   input resident, each step one captured launch graph: one predictor (one stream), and `inflight` predictors each on its own
   stream in flight at once as bench.py runs them.
Writes one JSON file and prints a table.  bench.py is not involved: G is opt-in and the benchmark runs the default program.
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, C, input plane, stride, M, tail): tail "res" = residual add + calib copy, "calib" = calib copy, "i8" = int8 output;
# drop = the fp32 sum has no consumer (the lowered program's -f32)
V2_BLOCKS = [
    ("b1", 32, 112, 1, 16, "i8", False), ("b2", 96, 112, 2, 24, "calib", False), ("b3", 144, 56, 1, 24, "res", True),
    ("b4", 144, 56, 2, 32, "calib", False), ("b5", 192, 28, 1, 32, "res", False), ("b6", 192, 28, 1, 32, "res", True),
    ("b7", 192, 28, 2, 64, "calib", False), ("b8", 384, 14, 1, 64, "res", False), ("b9", 384, 14, 1, 64, "res", False),
    ("b10", 384, 14, 1, 64, "res", True), ("b11", 384, 14, 1, 96, "calib", False), ("b12", 576, 14, 1, 96, "res", False),
    ("b13", 576, 14, 1, 96, "res", True), ("b14", 576, 14, 2, 160, "calib", False), ("b15", 960, 7, 1, 160, "res", False),
    ("b16", 960, 7, 1, 160, "res", True), ("b17", 960, 7, 1, 320, "i8", False),
]
HBM = 8e12


def block_case(ctx, capi, n, c, hw, s, m, tail, drop, reps):
    L = ctx.L
    oh = (hw + 2 - 3) // s + 1
    rng = np.random.default_rng(7)
    d_dw = capi.conv_desc(n, c, hw, hw, c, 3, 3, (1, 1, 1, 1), (s, s), (1, 1), c, capi.ACT_RELU6, 95.0)
    d_pw = capi.conv_desc(n, c, oh, oh, m, 1, 1)
    x = ctx.malloc(n * c * hw * hw)
    ctx.check(L.plhip_memset(ctx.h, x, 1, n * c * hw * hw), "memset")
    wdw = ctx.to_device(rng.integers(-127, 128, (c, 9)).astype(np.int8))
    sdw = ctx.to_device(np.full(c, 1e-3, np.float32))
    wraw = ctx.to_device(rng.integers(-127, 128, (m, c)).astype(np.int8))
    wp = ctx.malloc(L.plhip_conv_packed_weight_bytes(C.byref(d_pw)))
    ctx.check(L.plhip_pack_conv_weights(ctx.h, C.byref(d_pw), wraw, wp), "pack")
    spw = ctx.to_device(np.full(m, 1e-3, np.float32))
    cnt = n * m * oh * oh
    i8 = tail == "i8"
    y = ctx.malloc(cnt * (1 if i8 else 4))
    res = ctx.malloc(cnt * 4) if tail == "res" else C.c_void_p()
    if tail == "res":
        ctx.check(L.plhip_memset(ctx.h, res, 0, cnt * 4), "memset")
    yq = ctx.malloc(cnt) if not i8 else C.c_void_p()
    mid = ctx.malloc(n * c * oh * oh)
    kind = capi.OUT_I8 if i8 else capi.OUT_F32
    yo = C.c_void_p() if drop else y

    def fused():
        ctx.check(L.plhip_dw_conv1x1_fused_int8(ctx.h, C.byref(d_dw), x, wdw, sdw, None, m, wp, spw, None, 0, 0.0, yo, kind, res, 0,
                                                yq, 0.05), "fused")

    def two():
        ctx.check(L.plhip_depthwise_conv_int8(ctx.h, C.byref(d_dw), x, wdw, sdw, None, mid, capi.OUT_I8), "dw")
        if i8:
            ctx.check(L.plhip_conv2d_int8(ctx.h, C.byref(d_pw), mid, wp, spw, None, y, capi.OUT_I8, None, 0), "pw")
        else:
            ctx.check(L.plhip_conv2d_int8_fused(ctx.h, C.byref(d_pw), mid, wp, spw, None, yo, res, 0, yq, 0.05, None, 0), "pw")

    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ctx.check(L.plhip_event_create(ctx.h, C.byref(e)), "event")

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            L.plhip_event_record(ctx.h, ev[0])
            fn()
            L.plhip_event_record(ctx.h, ev[1])
            ctx.sync()
            ms = C.c_float()
            ctx.check(L.plhip_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)), "elapsed")
            ts.append(ms.value * 1e3)
        return float(np.median(ts))

    t_f, t_2 = timed(fused), timed(two)
    out_b = cnt * (1 if i8 else ((0 if drop else 4) + 1 + (4 if tail == "res" else 0)))
    b_f = n * c * hw * hw + out_b
    b_2 = b_f + 2 * n * c * oh * oh
    for e in ev:
        L.plhip_event_destroy(ctx.h, e)
    for p in [x, wdw, sdw, wraw, wp, spw, y, mid] + ([res] if tail == "res" else []) + ([yq] if not i8 else []):
        ctx.free(p)
    return dict(fused_us=round(t_f, 2), two_us=round(t_2, 2), ratio=round(t_f / t_2, 3), bytes_fused=b_f, bytes_two=b_2,
                frac_hbm_fused=round(b_f / (t_f * 1e-6) / HBM, 3), frac_hbm_two=round(b_2 / (t_2 * 1e-6) / HBM, 3))


def whole_graph(lite, wl, B, steps, inflight, rounds):
    net = wl.mobilenet_v2_net()
    img = np.random.default_rng(1000).uniform(-1, 1, (B, 3, 224, 224)).astype(np.float32)
    preds = {}
    for g in (False, True):
        ps = []
        for _ in range(inflight):
            p = lite.Predictor(0)
            wl.emit_graph(p, net, B, fuse=True, fuse_dwconv=g)
            p.graph_lower()
            p.set_input(net["input"], img)
            p.run()          # one-time work (packing, workspaces), uploads the input: resident from here on
            p.run_graph()    # records the launch graph
            p.sync()
            ps.append(p)
        preds[g] = ps

    def one_stream(g):
        p = preds[g][0]
        p.run_graph()
        p.sync()
        t = time.perf_counter()
        for _ in range(steps):
            p.run_graph()
        p.sync()
        return B * steps / (time.perf_counter() - t)

    def in_flight(g):
        ps = preds[g]
        for p in ps:
            p.run_graph()
        for p in ps:
            p.sync()
        per = max(1, steps // len(ps))

        def work(p):
            for _ in range(per):
                p.run_graph()
            p.sync()
        th = [threading.Thread(target=work, args=(p,)) for p in ps]
        t = time.perf_counter()
        for x in th:
            x.start()
        for x in th:
            x.join()
        return B * per * len(ps) / (time.perf_counter() - t)

    out = {"off": {"one_stream": [], "in_flight": []}, "on": {"one_stream": [], "in_flight": []}}
    for _ in range(rounds):
        for g in (False, True):
            k = "on" if g else "off"
            out[k]["one_stream"].append(round(one_stream(g)))
            out[k]["in_flight"].append(round(in_flight(g)))
    for ps in preds.values():
        for p in ps:
            p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/dwconv_g.json")
    ap.add_argument("--batches", default="1024,128")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip-graph", action="store_true")
    ap.add_argument("--graph-only", action="store_true", help="one G-on step loop only (for a kernel trace)")
    a = ap.parse_args()
    import importlib
    import __graft_entry__ as ge
    pkg = ge.import_package()
    capi = pkg.capi
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    if a.graph_only:
        net = wl.mobilenet_v2_net()
        p = lite.Predictor(0)
        wl.emit_graph(p, net, 1024, fuse=True, fuse_dwconv=True)
        p.graph_lower()
        p.set_input(net["input"], np.random.default_rng(1000).uniform(-1, 1, (1024, 3, 224, 224)).astype(np.float32))
        p.run()
        p.sync()
        p.run(skip_io_copy=True)
        p.sync()
        p.close()
        return
    res = {"blocks": {}}
    with capi.Context(0) as ctx:
        for B in [int(b) for b in a.batches.split(",")]:
            rows = []
            print("batch %d   block   C   plane s   M  tail   fused_us  two_us  ratio  fused_frac  two_frac" % B)
            for (name, c, hw, s, m, tail, drop) in V2_BLOCKS:
                r = block_case(ctx, capi, B, c, hw, s, m, tail, drop, a.reps)
                r.update(block=name, C=c, plane=hw, stride=s, M=m, tail=tail + ("-f32" if drop else ""))
                rows.append(r)
                print("%12s %5d %5d %d %4d %6s %9.1f %7.1f %6.3f %10.3f %9.3f" % (name, c, hw, s, m, r["tail"], r["fused_us"],
                                                                                   r["two_us"], r["ratio"], r["frac_hbm_fused"],
                                                                                   r["frac_hbm_two"]), flush=True)
            res["blocks"][str(B)] = rows
            res["blocks_sum_us_" + str(B)] = {"fused": round(sum(r["fused_us"] for r in rows), 1),
                                              "two": round(sum(r["two_us"] for r in rows), 1)}
    if not a.skip_graph:
        g = whole_graph(lite, wl, 1024, a.steps, a.inflight, a.rounds)
        res["c5_ab_img_per_s"] = g
        res["c5_ab_inflight"] = a.inflight
        print(json.dumps(g))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
