"""uint8 image input: what it costs and saves, in one process, variants alternated, medians.  Prints one JSON line (and writes it
to --out, e.g. profiles/image_feed_c3.json).

(a) the stem at MobileNetV1's shape, batch 128: conv3x3s2_mfma_f32in_kernel on the fp32 NCHW tensor (plhip_conv2d_calib_int8)
    against conv3x3s2_mfma_u8in_kernel on the uint8 BGR image (plhip_conv2d_image_int8), HIP events around each launch; and
    image_to_tensor_i8 at ResNet50's input shape (batch 128, 224 x 224 BGR) with its rate on algorithmic bytes (image in, int8 out);
(b) MobileNetV1 end to end at batch 128 with run(skip_io_copy=False): the fp32 feed against the uint8 feed, images/s with the
    host -> device copy inside the timing (bench.py measures the resident-input figure; it is not changed by this tool).

    python tools/imagefeed_bench.py [--reps 30] [--e2e-reps 20] [--out profiles/image_feed_c3.json]

With --frame HxW --frame-format FMT (both repeatable, paired in order; FMT: BGR, RGB, BGRA, RGBA, GRAY, NV12, NV21) it measures the
frame feed instead (profiles/frame_feed.json): per frame kind plhip_frame_to_tensor_i8 (one launch) against the separate launches
(convert for NV, resize, image_to_tensor_i8) with image_to_tensor_i8 at 128 x 224 x 224 BGR as the yardstick in the same loop, rates
over the algorithmic bytes (source rows actually touched: min(h_in, 2 h_out) rows, chroma rows likewise, + the int8 tensor); and
MobileNetV1 end to end (run(skip_io_copy=False)) fed the FIRST frame kind against the 224 x 224 BGR image feed.

    python tools/imagefeed_bench.py --frame 480x640 --frame-format NV12 --frame 1080x1920 --frame-format NV12 [--frame-batch 128]
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


FRAME_FORMATS = {"RGBA": 0, "BGRA": 1, "RGB": 2, "BGR": 3, "GRAY": 4, "NV21": 11, "NV12": 12}


def frame_kernels(capi, frames, batch, reps):
    """frames: [(h, w, format name)].  One process, every variant alternated inside one loop, medians."""
    rng = np.random.default_rng(4)
    ho = wo = 224
    cs = 1 / 127.0
    res = {"frame_batch": batch, "frames": []}
    with capi.Context(0) as ctx:
        L = ctx.L
        ev = _events(ctx)
        yard_src = ctx.to_device(rng.integers(0, 256, (128, ho, wo, 3)).astype(np.uint8))
        yard_img = capi.image_desc(128, ho, wo, capi.IMG_BGR, MEANS, SCALES)
        yard_q = ctx.malloc(128 * 3 * ho * wo)
        fns = {"yardstick_image_to_tensor_i8": lambda: ctx.check(L.plhip_image_to_tensor_i8(ctx.h, C.byref(yard_img), yard_src, yard_q, cs), "i2t")}
        meta = []
        for (h, w, name) in frames:
            fmt = FRAME_FORMATS[name]
            nv = fmt in (capi.IMG_NV12, capi.IMG_NV21)
            pcs = 3 if nv else capi.IMG_BYTES[fmt]
            shape = (batch, h * 3 // 2, w) if nv else (batch, h, w, pcs)
            dsrc = ctx.to_device(rng.integers(0, 256, shape).astype(np.uint8))
            fr = capi.frame_desc(batch, h, w, fmt)
            ifmt = capi.IMG_BGR if nv else fmt
            img = capi.image_desc(batch, ho, wo, ifmt, MEANS, SCALES)
            cout = capi.IMG_CHANNELS[ifmt]
            dq = ctx.malloc(batch * cout * ho * wo)
            dbgr = ctx.malloc(batch * h * w * 3) if nv else None
            dsmall = ctx.malloc(batch * ho * wo * pcs)
            bgr_fr = capi.frame_desc(batch, h, w, capi.IMG_BGR)
            key = "%dx%d_%s" % (h, w, name)

            def fused(fr=fr, img=img, dsrc=dsrc, dq=dq):
                ctx.check(L.plhip_frame_to_tensor_i8(ctx.h, C.byref(fr), C.byref(img), dsrc, dq, cs), "frame_to_tensor_i8")

            def separate(fr=fr, img=img, dsrc=dsrc, dq=dq, nv=nv, dbgr=dbgr, dsmall=dsmall, bgr_fr=bgr_fr):
                src, f = dsrc, fr
                if nv:
                    ctx.check(L.plhip_image_convert_u8(ctx.h, C.byref(fr), dsrc, capi.IMG_BGR, dbgr), "convert")
                    src, f = dbgr, bgr_fr
                ctx.check(L.plhip_image_resize_u8(ctx.h, C.byref(f), src, ho, wo, dsmall), "resize")
                ctx.check(L.plhip_image_to_tensor_i8(ctx.h, C.byref(img), dsmall, dq, cs), "i2t")

            fns[key + "/fused"] = fused
            fns[key + "/separate"] = separate
            rows = min(h, 2 * ho)
            alg = batch * (rows * w * (1 if nv else pcs) + (min(h // 2, 2 * ho) * w if nv else 0) + cout * ho * wo)
            meta.append((key, alg, int(np.prod(shape)) // batch))
        for f in fns.values():  # warm-up: also uploads the resize tables of every size
            f()
        ctx.sync()
        t = {k: [] for k in fns}
        for _ in range(reps):
            for k, f in fns.items():
                t[k].append(_time(ctx, ev, f))
        med = {k: statistics.median(v) for k, v in t.items()}
        res["yardstick_image_to_tensor_i8_128x224x224_BGR_us"] = round(med["yardstick_image_to_tensor_i8"], 2)
        for key, alg, fbytes in meta:
            fu, se = med[key + "/fused"], med[key + "/separate"]
            res["frames"].append({"frame": key, "bytes_per_frame": fbytes, "algorithmic_bytes": alg, "frame_to_tensor_i8_us": round(fu, 2),
                                  "frame_to_tensor_i8_TBps": round(alg / (fu * 1e-6) / 1e12, 3), "separate_launches_us": round(se, 2),
                                  "fusion_gain": round(se / fu, 3)})
        for e in ev:
            L.plhip_event_destroy(ctx.h, e)
    return res


def frame_end_to_end(pkg, frame, reps, batch=128):
    import importlib
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    net = wl.mobilenet_v1_net()
    rng = np.random.default_rng(5)
    h, w, name = frame
    fmt = FRAME_FORMATS[name]
    nv = fmt in (lite.IMG_NV12, lite.IMG_NV21)
    feeds = {"image": rng.integers(0, 256, (batch, 224, 224, 3)).astype(np.uint8),
             "frame": rng.integers(0, 256, (batch, h * 3 // 2, w) if nv else (batch, h, w, pkg.capi.IMG_BYTES[fmt])).astype(np.uint8)}
    preds = {}
    for kind in ("image", "frame"):
        p = lite.Predictor(0)
        if kind == "image":
            wl.emit_graph(p, net, batch, image=dict(format=lite.IMG_BGR, means=MEANS, scales=SCALES))
        else:
            wl.emit_graph(p, net, batch, frame=dict(h=h, w=w, format=fmt, means=MEANS, scales=SCALES))
        p.graph_lower()
        p.set_input(net["input"], feeds[kind])
        p.run()
        p.run()
        preds[kind] = p
    t = {"image": [], "frame": []}
    for _ in range(reps):
        for kind in ("image", "frame"):
            p = preds[kind]
            t0 = time.perf_counter()
            p.set_input(net["input"], feeds[kind])
            p.run(skip_io_copy=False)
            p.sync()
            t[kind].append(time.perf_counter() - t0)
    for p in preds.values():
        p.close()
    return {"e2e_batch": batch, "e2e_frame": "%dx%d_%s" % (h, w, name), "e2e_image_feed_img_s": round(batch / statistics.median(t["image"]), 1),
            "e2e_frame_feed_img_s": round(batch / statistics.median(t["frame"]), 1), "e2e_image_feed_bytes": int(feeds["image"].nbytes),
            "e2e_frame_feed_bytes": int(feeds["frame"].nbytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--e2e-reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--frame", action="append", default=[], help="HxW of a source frame (repeatable): measures the frame feed instead")
    ap.add_argument("--frame-format", action="append", default=[], help="format of the matching --frame (default NV12)")
    ap.add_argument("--frame-batch", type=int, default=128)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.import_package()
    res = {"tool": "imagefeed_bench", "device": "MI355X"}
    if a.frame:
        fmts = a.frame_format + ["NV12"] * (len(a.frame) - len(a.frame_format))
        frames = [tuple(int(v) for v in f.lower().split("x")) + (fmts[i].upper(),) for i, f in enumerate(a.frame)]
        res.update(frame_kernels(pkg.capi, frames, a.frame_batch, a.reps))
        if a.e2e_reps > 0:
            res.update(frame_end_to_end(pkg, frames[0], a.e2e_reps))
    else:
        res.update(stem_and_stream(pkg.capi, a.reps))
        res.update(end_to_end(pkg, a.e2e_reps))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
