#!/usr/bin/env python3
"""Detection heads on the device: what multiclass_nms and the tiled transpose cost and what fusion O saves.  One
process, the variants alternated in one loop, device events on one stream, warm-up stated.  Prints one JSON line and writes it to
--out.

(a) ssd_mini_net, batch 32, 300 x 300, one step in flight (run(skip_io_copy=True), resident input): the default fusions with O off,
    O on, O off again, alternating; --steps rounds after --warmup steps each.  The off program is timed TWICE per round (off_a,
    off_b): the spread between two runs of the same program is what a difference has to beat.
(b) --kernels: plhip_multiclass_nms_f32 alone at SSD300's shape (N 32, C 21, P 1917, top 400, keep 200) and YOLOv3-416's (N 8, C 80,
    P 10647, top 1000, keep 100), on clustered boxes and scores of which about 5 % pass the threshold, in both score layouts; and
    plhip_transpose_f32 on the tiled kernel ((0,2,3,1) of an SSD conf head [32, 126, 19, 19], (0,2,1) of [32, 1917, 21], and a
    square [32, 512, 512] that takes the quad path) against plhip_calib_i8_to_f32 moving as many bytes, the stream yardstick of
    DESIGN.md 13.  --inner launches between two events.

    python tools/detbench.py [--steps 20] [--warmup 5] [--batch 32] [--res 300] [--kernels] [--out profiles/detection.json]
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

# (tag, N, C, P, nms_top_k, keep_top_k)
NMS_SHAPES = (("ssd300", 32, 21, 1917, 400, 200), ("yolov3_416", 8, 80, 10647, 1000, 100))
# (tag, dims, perm)
TRANSPOSE_SHAPES = (("conf_head_nchw_to_nhwc", (32, 126, 19, 19), (0, 2, 3, 1)), ("scores_npc_to_ncp", (32, 1917, 21), (0, 2, 1)),
                    ("square_512_quads", (32, 512, 512), (0, 2, 1)))


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


def network(capi, lite, wl, batch, res_px, steps, warmup):
    net = wl.ssd_mini_net(res=res_px)
    img = np.random.default_rng(5).uniform(-1, 1, (batch, 3, res_px, res_px)).astype(np.float32)
    modes = {"off_a": dict(fuse=True, fuse_detection_head=False), "o_on": dict(fuse=True, fuse_detection_head=True),
             "off_b": dict(fuse=True, fuse_detection_head=False)}
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
                p.run()
                for _ in range(warmup):
                    p.run(skip_io_copy=True)
                p.sync()
            ref = preds["off_a"].get_var("det", np.float32), preds["off_a"].get_var("det/count", np.int32)
            same = bool(ref[0].tobytes() == preds["o_on"].get_var("det", np.float32).tobytes() and
                        ref[1].tobytes() == preds["o_on"].get_var("det/count", np.int32).tobytes())
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
    # per-round differences: the same program against itself (the spread) and O against the mean of the two off runs
    self_diff = [abs(a - b) for a, b in zip(t["off_a"], t["off_b"])]
    spread = max(statistics.median(self_diff), abs(off_a - off_b))
    res["off_spread_ms"] = dict(median_abs_diff=round(statistics.median(self_diff), 4), max_abs_diff=round(max(self_diff), 4),
                                medians_diff=round(abs(off_a - off_b), 4))
    gain = [(a + b) / 2 - o for a, b, o in zip(t["off_a"], t["off_b"], t["o_on"])]
    res["o_on_gain_ms"] = dict(median=round(statistics.median(gain), 4), min=round(min(gain), 4), max=round(max(gain), 4))
    # the rule of DESIGN.md 14: faster in EVERY round, by more than the off-vs-off spread
    res["o_on_beats_spread"] = bool(min(gain) > spread)
    res["detections_identical"] = same
    res["priors"] = int(net["shapes"]["priors"][0])
    return res


def _nms_inputs(rng, n, c, p):
    """Boxes in clusters of about six; about 5 % of the scores above the 0.01 threshold."""
    centres = rng.random((n, max(1, p // 6), 2)).astype(np.float32)
    which = rng.integers(0, centres.shape[1], (n, p))
    ctr = np.take_along_axis(centres, which[..., None].repeat(2, -1), axis=1) + (rng.standard_normal((n, p, 2)) * 0.02).astype(np.float32)
    half = (0.03 + 0.05 * rng.random((n, p, 2))).astype(np.float32)
    boxes = np.concatenate([ctr - half, ctr + half], axis=-1).astype(np.float32)
    u = rng.random((n, c, p)).astype(np.float32)
    scores = np.where(u < 0.05, np.float32(0.01) + u * np.float32(10), u * np.float32(0.009)).astype(np.float32)
    return boxes, scores


def kernels(capi, reps, inner):
    rng = np.random.default_rng(11)
    res = {}
    with capi.Context(0) as ctx:
        L, h, ck = ctx.L, ctx.h, ctx.check
        ev = _events(ctx)
        for tag, n, c, p, top, keep in NMS_SHAPES:
            boxes, scores = _nms_inputs(rng, n, c, p)
            db = ctx.to_device(boxes)
            out, idx, cnt = ctx.malloc(4 * n * keep * 6), ctx.malloc(4 * n * keep), ctx.malloc(4 * n)
            r = {}
            for layout in ("ncp", "npc"):
                d = capi.nms_desc(n, c, p, 0, 0.01, top, 0.45, keep, layout=layout)
                ws = ctx.malloc(L.plhip_multiclass_nms_workspace_bytes(C.byref(d)))
                ds = ctx.to_device(scores if layout == "ncp" else np.ascontiguousarray(scores.transpose(0, 2, 1)))
                fn = lambda: ck(L.plhip_multiclass_nms_f32(h, db, ds, C.byref(d), ws, out, idx, cnt), "nms")
                fn(), fn()
                ctx.sync()
                t = [_timed_ms(ctx, ev, fn, inner) * 1e3 for _ in range(reps)]
                kept = ctx.to_host(cnt, (n,), np.int32)
                r[layout] = dict(_stat(t, "us", 2), detections_per_image=round(float(kept.mean()), 1),
                                 candidates_per_class=round(float((scores[:, 1:] > 0.01).sum(axis=2).mean()), 1))
                ctx.free(ws), ctx.free(ds)
            res["nms_" + tag] = r
            for q in (db, out, idx, cnt):
                ctx.free(q)
        for tag, dims, perm in TRANSPOSE_SHAPES:
            cnt = int(np.prod(dims))
            x = ctx.to_device(rng.standard_normal(cnt).astype(np.float32))
            y, q8 = ctx.malloc(4 * cnt), ctx.malloc(2 * cnt)
            ck(L.plhip_memset(h, q8, 1, 2 * cnt), "memset")
            cd, cp = (C.c_int64 * len(dims))(*dims), (C.c_int * len(perm))(*perm)
            # the yardstick moves the same 8 bytes per element: 2 int8 elements in, 2 fp32 elements out per 10 bytes is the nearest the
            # stream kernel gets, so it is run on 8 / 5 of the element count
            ycnt = (8 * cnt // 5) // 4 * 4
            ybuf = ctx.malloc(4 * ycnt)
            variants = {"transpose": lambda: ck(L.plhip_transpose_f32(h, x, cd, cp, len(dims), y), "transpose"),
                        "stream_i8_to_f32": lambda: ck(L.plhip_calib_i8_to_f32(h, q8, ybuf, 0.03, ycnt), "calib")}
            for fn in variants.values():
                fn(), fn()
            ctx.sync()
            t = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    t[k].append(_timed_ms(ctx, ev, fn, inner) * 1e3)
            nb = {"transpose": 8 * cnt, "stream_i8_to_f32": 5 * ycnt}
            r = {k: dict(_stat(v, "us", 3), algorithmic_bytes=nb[k], tb_per_s=round(nb[k] / statistics.median(v) / 1e6, 3)) for k, v in t.items()}
            r["transpose_over_stream"] = round(r["transpose"]["median_us"] / r["stream_i8_to_f32"]["median_us"], 3)
            res["transpose_" + tag] = r
            for q in (x, y, q8, ybuf):
                ctx.free(q)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=300)
    ap.add_argument("--kernels", action="store_true", help="also time the NMS and the transpose")
    ap.add_argument("--kernels-only", action="store_true", help="part (b) alone")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.import_package()
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    out = dict(tool="detbench", model="ssd_mini", batch=a.batch, res=a.res, steps=a.steps,
               warmup="%d steps per program; 2 launches per kernel variant" % a.warmup)
    if not a.kernels_only:
        out["network"] = network(pkg.capi, lite, wl, a.batch, a.res, a.steps, a.warmup)
    if a.kernels or a.kernels_only:
        out["kernels"] = kernels(pkg.capi, a.reps, a.inner)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
