"""uint8 image input: what it costs and saves, in one process, variants alternated, medians.  Prints one JSON line (and writes it
to --out, e.g. profiles/image_feed_c3.json).

(a) the stem at MobileNetV1's shape, batch 128: conv3x3s2_mfma_f32in_kernel on the fp32 NCHW tensor (plhip_conv2d_calib_int8)
    against conv3x3s2_mfma_u8in_kernel on the uint8 BGR image (plhip_conv2d_image_int8), HIP events around each launch; and
    image_to_tensor_i8 at ResNet50's input shape (batch 128, 224 x 224 BGR) with its rate on algorithmic bytes (image in, int8 out);
(b) MobileNetV1 end to end at batch 128 with run(skip_io_copy=False): the fp32 feed against the uint8 feed, images/s with the
    host -> device copy inside the timing (bench.py measures the resident-input figure; it is not changed by this tool).

    python tools/imagefeed_bench.py [--reps 30] [--e2e-reps 20] [--out profiles/image_feed_c3.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEANS = (120.0, 127.5, 135.0)
SCALES = (1 / 127.5 * 1.03, 1 / 127.5, 1 / 127.5 * 0.97)


def _events(ctx):
    a, b = C.c_void_p(), C.c_void_p()
    ctx.check(ctx.L.plhip_event_create(ctx.h, C.byref(a)), "event")
    ctx.check(ctx.L.plhip_event_create(ctx.h, C.byref(b)), "event")
    return a, b


def _time(ctx, ev, fn):
    ctx.check(ctx.L.plhip_event_record(ctx.h, ev[0]), "record")
    fn()
    ctx.check(ctx.L.plhip_event_record(ctx.h, ev[1]), "record")
    ctx.sync()
    ms = C.c_float()
    ctx.check(ctx.L.plhip_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)), "elapsed")
    return ms.value * 1e3


def stem_and_stream(capi, reps):
    rng = np.random.default_rng(3)
    n, h, w, cout = 128, 224, 224, 32
    res = {}
    with capi.Context(0) as ctx:
        L = ctx.L
        ev = _events(ctx)
        src = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
        xf = ((src.astype(np.float32).transpose(0, 3, 1, 2) - np.float32(127.5)) * np.float32(1 / 127.5)).copy()
        img = capi.image_desc(n, h, w, capi.IMG_BGR, MEANS, SCALES)
        d = capi.conv_desc(n, 3, h, w, cout, 3, 3, (1, 1, 1, 1), (2, 2), act=capi.ACT_RELU)
        dsrc, dxf = ctx.to_device(src), ctx.to_device(xf)
        wt = rng.integers(-127, 128, (cout, 3, 3, 3)).astype(np.int8)
        dw = ctx.to_device(wt)
        dwp = ctx.malloc(L.plhip_conv_packed_weight_bytes(C.byref(d)))
        ctx.check(L.plhip_pack_conv_weights(ctx.h, C.byref(d), dw, dwp), "pack")
        dsc = ctx.to_device(np.full(cout, 0.01, np.float32))
        dy = ctx.malloc(n * cout * 112 * 112)
        dq = ctx.malloc(n * 3 * h * w)
        cs = 1 / 127.0

        def f32in():
            ctx.check(L.plhip_conv2d_calib_int8(ctx.h, C.byref(d), dxf, cs, dwp, dsc, None, dy, capi.OUT_I8), "f32in")

        def u8in():
            ctx.check(L.plhip_conv2d_image_int8(ctx.h, C.byref(d), C.byref(img), dsrc, cs, dwp, dsc, None, dy, capi.OUT_I8), "u8in")

        def i2t():
            ctx.check(L.plhip_image_to_tensor_i8(ctx.h, C.byref(img), dsrc, dq, cs), "image_to_tensor_i8")

        for f in (f32in, u8in, i2t):  # warm-up
            f()
        ctx.sync()
        t = {"f32in": [], "u8in": [], "i2t": []}
        for _ in range(reps):  # alternated
            t["f32in"].append(_time(ctx, ev, f32in))
            t["u8in"].append(_time(ctx, ev, u8in))
            t["i2t"].append(_time(ctx, ev, i2t))
        med = {k: statistics.median(v) for k, v in t.items()}
        alg = 2 * n * h * w * 3  # image bytes in + int8 tensor out
        res["stem_f32in_us"] = round(med["f32in"], 2)
        res["stem_u8in_us"] = round(med["u8in"], 2)
        res["stem_speedup"] = round(med["f32in"] / med["u8in"], 3)
        res["image_to_tensor_i8_us"] = round(med["i2t"], 2)
        res["image_to_tensor_i8_TBps"] = round(alg / (med["i2t"] * 1e-6) / 1e12, 3)
        res["image_to_tensor_i8_frac_of_8TBps"] = round(res["image_to_tensor_i8_TBps"] / 8.0, 3)
        for e in ev:
            L.plhip_event_destroy(ctx.h, e)
    return res


def end_to_end(pkg, reps, batch=128):
    import importlib
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    net = wl.mobilenet_v1_net()
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (batch, 224, 224, 3)).astype(np.uint8)
    xf = ((src.astype(np.float32) - np.float32(MEANS)) * np.float32(SCALES)).transpose(0, 3, 1, 2).copy()
    preds = {}
    for kind in ("fp32", "uint8"):
        p = lite.Predictor(0)
        wl.emit_graph(p, net, batch, image=None if kind == "fp32" else dict(format=lite.IMG_BGR, means=MEANS, scales=SCALES))
        p.graph_lower()
        feed = xf if kind == "fp32" else src
        p.set_input(net["input"], feed)
        p.run()
        p.run()
        preds[kind] = (p, feed)
    t = {"fp32": [], "uint8": []}
    for _ in range(reps):
        for kind in ("fp32", "uint8"):
            p, feed = preds[kind]
            t0 = time.perf_counter()
            p.set_input(net["input"], feed)  # host-side copy into the feed tensor, then the program with its io_copy
            p.run(skip_io_copy=False)
            p.sync()
            t[kind].append(time.perf_counter() - t0)
    for p, _ in preds.values():
        p.close()
    return {"e2e_batch": batch, "e2e_fp32_feed_img_s": round(batch / statistics.median(t["fp32"]), 1),
            "e2e_uint8_feed_img_s": round(batch / statistics.median(t["uint8"]), 1),
            "e2e_fp32_feed_bytes": int(xf.nbytes), "e2e_uint8_feed_bytes": int(src.nbytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--e2e-reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.import_package()
    res = {"tool": "imagefeed_bench", "device": "MI355X"}
    res.update(stem_and_stream(pkg.capi, a.reps))
    res.update(end_to_end(pkg, a.e2e_reps))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
