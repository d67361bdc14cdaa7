#!/usr/bin/env python3
"""A YOLOv3 head on the device: what fusion P saves and what the one-launch head costs.  The method of
tools/detbench.py: one process, the variants alternated in one loop, device events on one stream, warm-up stated.
Prints one JSON line and writes it to --out.

(a) yolov3_mini_net, batch 8, 416 x 416, 80 classes (P 10647, YOLOv3-416's head), one step in flight (run(skip_io_copy=True),
    resident inputs): the default fusions with P off, P on, P off again, alternating; --steps rounds after --warmup steps each.  The
    off program is timed TWICE per round (off_a, off_b): the spread between two runs of the same program is what a difference has
    to beat.  The rule, set in advance: P is on by default only if it is faster in EVERY round by more than that spread.
(b) --kernels: plhip_yolo_head_f32 alone at that shape (N 8, C 80, maps 13 / 26 / 52 with 3 anchors each), the separate launches it
    replaces (plhip_yolo_box_f32 x 3 -> plhip_concat_f32 x 2 -> plhip_transpose_f32), and plhip_calib_i8_to_f32 moving as many
    bytes as the head does, the stream yardstick of DESIGN.md 13.  --inner launches between two events.

    python tools/yolobench.py [--steps 20] [--warmup 5] [--batch 8] [--res 416] [--classes 80] [--kernels] [--out profiles/yolo.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events(ctx):
    a, b = C.c_void_p(), C.c_void_p()
    ctx.check(ctx.L.plhip_event_create(ctx.h, C.byref(a)), "event")
    ctx.check(ctx.L.plhip_event_create(ctx.h, C.byref(b)), "event")
    return a, b


def _timed_ms(ctx, ev, fn, inner=1):
    ctx.check(ctx.L.plhip_event_record(ctx.h, ev[0]), "record")
    for _ in range(inner):
        fn()
    ctx.check(ctx.L.plhip_event_record(ctx.h, ev[1]), "record")
    ctx.sync()
    ms = C.c_float()
    ctx.check(ctx.L.plhip_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)), "elapsed")
    return ms.value / inner


def _stat(v, unit="ms", digits=4):
    return {"median_" + unit: round(statistics.median(v), digits), "min_" + unit: round(min(v), digits), "max_" + unit: round(max(v), digits)}


def network(capi, lite, wl, batch, res_px, classes, steps, warmup):
    net = wl.yolov3_mini_net(res=res_px, num_classes=classes)
    rng = np.random.default_rng(5)
    img = rng.uniform(-1, 1, (batch, 3, res_px, res_px)).astype(np.float32)
    size = np.stack([rng.integers(300, 800, batch), rng.integers(300, 800, batch)], axis=1).astype(np.int32)
    modes = {"off_a": dict(fuse=True, fuse_yolo_head=False), "p_on": dict(fuse=True, fuse_yolo_head=True),
             "off_b": dict(fuse=True, fuse_yolo_head=False)}
    with capi.Context(0) as ctx:
        stream = ctx.L.plhip_ctx_stream(ctx.h)
        ev = _events(ctx)
        preds = {}
        try:
            for m, kw in modes.items():
                p = lite.Predictor(0, stream=stream)  # the events and every predictor share one stream
                preds[m] = p
                wl.emit_graph(p, net, batch, **kw)
                p.graph_lower()
                p.set_input(net["input"], img)
                p.set_input(net["img_size"], size)
                p.run()
                for _ in range(warmup):
                    p.run(skip_io_copy=True)
                p.sync()
            ref = preds["off_a"].get_var("det", np.float32), preds["off_a"].get_var("det/count", np.int32)
            same = bool(ref[0].tobytes() == preds["p_on"].get_var("det", np.float32).tobytes() and
                        ref[1].tobytes() == preds["p_on"].get_var("det/count", np.int32).tobytes())
            t = {m: [] for m in modes}
            for _ in range(steps):
                for m, p in preds.items():
                    t[m].append(_timed_ms(ctx, ev, lambda p=p: p.run(skip_io_copy=True)))
            res = {m: dict(_stat(v), img_per_s=round(batch / statistics.median(v) * 1e3, 1), instructions=preds[m].num_instructions())
                   for m, v in t.items()}
        finally:
            for p in preds.values():
                p.close()
    off_a, off_b = res["off_a"]["median_ms"], res["off_b"]["median_ms"]
    # per-round differences: the same program against itself (the spread) and P against the mean of the two off runs
    self_diff = [abs(a - b) for a, b in zip(t["off_a"], t["off_b"])]
    spread = max(statistics.median(self_diff), abs(off_a - off_b))
    res["off_spread_ms"] = dict(median_abs_diff=round(statistics.median(self_diff), 4), max_abs_diff=round(max(self_diff), 4),
                                medians_diff=round(abs(off_a - off_b), 4))
    gain = [(a + b) / 2 - o for a, b, o in zip(t["off_a"], t["off_b"], t["p_on"])]
    res["p_on_gain_ms"] = dict(median=round(statistics.median(gain), 4), min=round(min(gain), 4), max=round(max(gain), 4))
    # the rule of DESIGN.md 14 and 16: faster in EVERY round, by more than the off-vs-off spread
    res["p_on_beats_spread"] = bool(min(gain) > spread)
    res["detections_identical"] = same
    res["detections_per_image"] = [int(v) for v in ref[1]]
    res["priors"] = int(net["shapes"]["boxes"][0])
    return res


def kernels(capi, wl, batch, res_px, classes, reps, inner):
    rng = np.random.default_rng(11)
    maps = [res_px // 32, res_px // 16, res_px // 8]
    ratios = [32, 16, 8]
    anchors = [list(wl.COCO_ANCHORS[12:18]), list(wl.COCO_ANCHORS[6:12]), list(wl.COCO_ANCHORS[0:6])]
    ch = 3 * (5 + classes)
    with capi.Context(0) as ctx:
        L, h, ck = ctx.L, ctx.h, ctx.check
        ev = _events(ctx)
        shapes = [(batch, ch, m, m) for m in maps]
        xs = []
        for s in shapes:
            x = (rng.standard_normal(s) * 2).astype(np.float32).reshape(batch, 3, 5 + classes, -1)
            x[:, :, 4] -= np.float32(4)   # most cells below conf_thresh, as in a trained head
            xs.append(ctx.to_device(x))
        img = ctx.to_device(np.full((batch, 2), res_px, np.int32))
        ps = [3 * m * m for m in maps]
        P = sum(ps)
        boxes, scores = ctx.malloc(4 * batch * P * 4), ctx.malloc(4 * batch * P * classes)
        sb = [ctx.malloc(4 * batch * p * 4) for p in ps]
        ss = [ctx.malloc(4 * batch * p * classes) for p in ps]
        jb, js, jt = ctx.malloc(4 * batch * P * 4), ctx.malloc(4 * batch * P * classes), ctx.malloc(4 * batch * P * classes)

        def head():
            ck(ctx.yolo_head_launch(xs, img, shapes, anchors, classes, 0.01, ratios, True, 1.0, boxes, scores), "yolo_head")

        ext = (C.c_int64 * 3)(*ps)
        pb, pscore = (C.c_void_p * 3)(*sb), (C.c_void_p * 3)(*ss)
        dims, perm = (C.c_int64 * 3)(batch, P, classes), (C.c_int * 3)(0, 2, 1)

        def separate():
            for i in range(3):
                ck(ctx.yolo_box_launch(xs[i], img, shapes[i], anchors[i], classes, 0.01, ratios[i], True, 1.0, sb[i], ss[i]), "yolo_box")
            ck(L.plhip_concat_f32(h, pb, ext, 3, batch, 4, jb), "concat")
            ck(L.plhip_concat_f32(h, pscore, ext, 3, batch, classes, js), "concat")
            ck(L.plhip_transpose_f32(h, js, dims, perm, 3, jt), "transpose")

        nbytes = batch * P * 4 * ((5 + classes) + (4 + classes))   # every entry read once, every box and score written once
        ycnt = (nbytes // 5) // 4 * 4
        q8, ybuf = ctx.malloc(ycnt), ctx.malloc(4 * ycnt)
        ck(L.plhip_memset(h, q8, 1, ycnt), "memset")
        variants = {"yolo_head": head, "separate_6_launches": separate,
                    "stream_i8_to_f32": lambda: ck(L.plhip_calib_i8_to_f32(h, q8, ybuf, 0.03, ycnt), "calib")}
        for fn in variants.values():
            fn(), fn()
        ctx.sync()
        same = bool(ctx.to_host(scores, (batch * classes * P,), np.uint32).tobytes() == ctx.to_host(jt, (batch * classes * P,), np.uint32).tobytes() and
                    ctx.to_host(boxes, (batch * P * 4,), np.uint32).tobytes() == ctx.to_host(jb, (batch * P * 4,), np.uint32).tobytes())
        t = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                t[k].append(_timed_ms(ctx, ev, fn, inner) * 1e3)
        res = {k: _stat(v, "us", 3) for k, v in t.items()}
        res["yolo_head"].update(algorithmic_bytes=nbytes, tb_per_s=round(nbytes / res["yolo_head"]["median_us"] / 1e6, 3))
        res["stream_i8_to_f32"].update(algorithmic_bytes=5 * ycnt, tb_per_s=round(5 * ycnt / res["stream_i8_to_f32"]["median_us"] / 1e6, 3))
        res["head_over_stream"] = round(res["yolo_head"]["median_us"] / res["stream_i8_to_f32"]["median_us"], 3)
        res["separate_over_head"] = round(res["separate_6_launches"]["median_us"] / res["yolo_head"]["median_us"], 3)
        res["outputs_identical"] = same
        res["shape"] = dict(n=batch, classes=classes, maps=maps, priors=P)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=416)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--kernels", action="store_true", help="also time the head launch alone")
    ap.add_argument("--kernels-only", action="store_true", help="part (b) alone")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.import_package()
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    out = dict(tool="yolobench", model="yolov3_mini", batch=a.batch, res=a.res, classes=a.classes, steps=a.steps,
               warmup="%d steps per program; 2 launches per kernel variant" % a.warmup)
    if not a.kernels_only:
        out["network"] = network(pkg.capi, lite, wl, a.batch, a.res, a.classes, a.steps, a.warmup)
    if a.kernels or a.kernels_only:
        out["kernels"] = kernels(pkg.capi, wl, a.batch, a.res, a.classes, a.reps, a.inner)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
