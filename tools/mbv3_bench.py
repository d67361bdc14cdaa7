"""MobileNetV3 on the device: what the rewrites J1 / J2 / J3 cost and save.  One process, every variant alternated
in one loop, medians, warm-up stated.  Prints one JSON line and writes it to --out (profiles/mbv3.json).

(a) MobileNetV3-Large and -Small, batch 128, images/s with one step in flight (run(skip_io_copy=True) + sync, resident input):
    the unfused lowering, the builder's default fusions, and the default fusions with J1 / J2 / J3; 3 warm-up steps each.
(b) per rewrite, the launches it replaces against the one launch, HIP events around --inner back-to-back launches, at the largest
    and the smallest shape the rewrite occurs at in the two networks (batch 128):
      J1  hard_swish f32 + calib            vs  hard_swish int8 (and the both-outputs form)
      J3  se_scale f32 + calib              vs  se_scale int8
      J2  calib + conv 1x1 + conv 1x1 + hard_sigmoid   vs  se_gate
    microseconds and, for the two streams, TB/s over algorithmic bytes (fp32 in, int8 out; + fp32 out for the both form) beside
    image_to_tensor_i8 at 128 x 224 x 224 BGR, the yardstick of DESIGN.md 9, measured in the same loop.

    python tools/mbv3_bench.py [--reps 15] [--inner 20] [--steps 12] [--out profiles/mbv3.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events(ctx):
    a, b = C.c_void_p(), C.c_void_p()
    ctx.check(ctx.L.plhip_event_create(ctx.h, C.byref(a)), "event")
    ctx.check(ctx.L.plhip_event_create(ctx.h, C.byref(b)), "event")
    return a, b


def _time_us(ctx, ev, fn, inner):
    ctx.check(ctx.L.plhip_event_record(ctx.h, ev[0]), "record")
    for _ in range(inner):
        fn()
    ctx.check(ctx.L.plhip_event_record(ctx.h, ev[1]), "record")
    ctx.sync()
    ms = C.c_float()
    ctx.check(ctx.L.plhip_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)), "elapsed")
    return ms.value * 1e3 / inner


def _alternate(ctx, variants, reps, inner):
    """variants: {name: fn}.  Warm-up: 2 launches of each; then reps rounds, every variant once per round."""
    ev = _events(ctx)
    for fn in variants.values():
        fn(), fn()
    ctx.sync()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(_time_us(ctx, ev, fn, inner))
    return {k: dict(median_us=round(statistics.median(v), 3), min_us=round(min(v), 3), max_us=round(max(v), 3)) for k, v in t.items()}


def rewrites(capi, reps, inner):
    rng = np.random.default_rng(11)
    res = {}
    with capi.Context(0) as ctx:
        L, h = ctx.L, ctx.h
        ck = ctx.check
        swish = (C.c_float * 3)(6, 6, 3)
        sigm = (C.c_float * 3)(0.2, 0.5, 0)
        null = C.c_void_p()
        # the yardstick
        img = capi.image_desc(128, 224, 224, capi.IMG_BGR, (120.0, 127.5, 135.0), (1 / 127.5,) * 3)
        src = ctx.to_device(rng.integers(0, 256, (128, 224, 224, 3)).astype(np.uint8))
        dst = ctx.malloc(128 * 3 * 224 * 224)
        variants = {"image_to_tensor_i8": lambda: ck(L.plhip_image_to_tensor_i8(h, C.byref(img), src, dst, 1 / 127.0), "i2t")}
        nbytes = {"image_to_tensor_i8": 128 * 224 * 224 * 3 * 2}
        # J1: the stem's tensor (both forms) and the head's [128, 1280]; J3: 72 x 28 x 28 (Large b4) and 960 x 7 x 7 (Large b14 / b15)
        for tag, cnt in (("j1_16x112x112", 128 * 16 * 112 * 112), ("j1_1280x1x1", 128 * 1280)):
            x = ctx.to_device((rng.standard_normal(cnt) * 3).astype(np.float32))
            yf, yq = ctx.malloc(cnt * 4), ctx.malloc(cnt)

            def sep(x=x, yf=yf, yq=yq, cnt=cnt):
                ck(L.plhip_hard_act_f32(h, 0, swish, x, yf, null, 1.0, cnt), "hs")
                ck(L.plhip_calib_f32_to_i8(h, yf, yq, 0.09, cnt), "calib")
            variants[tag + "/separate"] = sep
            variants[tag + "/int8"] = lambda x=x, yq=yq, cnt=cnt: ck(L.plhip_hard_act_f32(h, 0, swish, x, null, yq, 0.09, cnt), "hs8")
            variants[tag + "/both"] = lambda x=x, yf=yf, yq=yq, cnt=cnt: ck(L.plhip_hard_act_f32(h, 0, swish, x, yf, yq, 0.09, cnt), "hsb")
            nbytes[tag + "/separate"] = nbytes[tag + "/int8"] = cnt * 5
            nbytes[tag + "/both"] = cnt * 9
        for tag, c, hw in (("j3_72x28x28", 72, 784), ("j3_960x7x7", 960, 49)):
            cnt = 128 * c * hw
            x = ctx.to_device((rng.standard_normal(cnt) * 3).astype(np.float32))
            g = ctx.to_device(rng.uniform(0, 1, 128 * c).astype(np.float32))
            yf, yq = ctx.malloc(cnt * 4), ctx.malloc(cnt)

            def sep(x=x, g=g, yf=yf, yq=yq, c=c, hw=hw, cnt=cnt):
                ck(L.plhip_se_scale_f32(h, x, g, 128, c, hw, yf, null, 1.0), "mul")
                ck(L.plhip_calib_f32_to_i8(h, yf, yq, 0.09, cnt), "calib")
            variants[tag + "/separate"] = sep
            variants[tag + "/int8"] = lambda x=x, g=g, yq=yq, c=c, hw=hw: ck(L.plhip_se_scale_f32(h, x, g, 128, c, hw, null, yq, 0.09), "mul8")
            nbytes[tag + "/separate"] = nbytes[tag + "/int8"] = cnt * 5
        # J2: (960, 240) and (16, 8)
        for c, cr in ((960, 240), (16, 8)):
            tag = "j2_%d_%d" % (c, cr)
            n = 128
            pooled = ctx.to_device(rng.uniform(0, 3, (n, c)).astype(np.float32))
            w1 = ctx.to_device(rng.integers(-127, 128, (cr, c)).astype(np.int8))
            w2 = ctx.to_device(rng.integers(-127, 128, (c, cr)).astype(np.int8))
            s1, b1 = ctx.to_device(np.full(cr, 1e-4, np.float32)), ctx.to_device(np.zeros(cr, np.float32))
            s2, b2 = ctx.to_device(np.full(c, 2e-4, np.float32)), ctx.to_device(np.zeros(c, np.float32))
            d1 = capi.conv_desc(n, c, 1, 1, cr, 1, 1, act=capi.ACT_RELU)
            d2 = capi.conv_desc(n, cr, 1, 1, c, 1, 1)
            wp1, wp2 = ctx.malloc(L.plhip_conv_packed_weight_bytes(C.byref(d1))), ctx.malloc(L.plhip_conv_packed_weight_bytes(C.byref(d2)))
            ck(L.plhip_pack_conv_weights(h, C.byref(d1), w1, wp1), "pack")
            ck(L.plhip_pack_conv_weights(h, C.byref(d2), w2, wp2), "pack")
            wsb = max(L.plhip_conv_workspace_bytes(C.byref(d1)), L.plhip_conv_workspace_bytes(C.byref(d2)))
            ws = ctx.malloc(wsb) if wsb else null
            gp = ctx.malloc(L.plhip_se_gate_packed_weight_bytes(c, cr))
            ck(L.plhip_pack_se_gate_weights(h, c, cr, w1, w2, gp), "pack_gate")
            q, mid, y, gate = ctx.malloc(n * c), ctx.malloc(n * cr), ctx.malloc(n * c * 4), ctx.malloc(n * c * 4)
            gd = capi.SeGateDesc(n, c, cr, 0.025, capi.ACT_RELU, capi.ACT_NONE, 0.0, 0.0, 0.2, 0.5)

            def sep(pooled=pooled, q=q, mid=mid, y=y, gate=gate, d1=d1, d2=d2, wp1=wp1, wp2=wp2, s1=s1, b1=b1, s2=s2, b2=b2, ws=ws, wsb=wsb, n=n, c=c):
                ck(L.plhip_calib_f32_to_i8(h, pooled, q, 0.025, n * c), "calib")
                ck(L.plhip_conv2d_int8(h, C.byref(d1), q, wp1, s1, b1, mid, capi.OUT_I8, ws, wsb), "conv1")
                ck(L.plhip_conv2d_int8(h, C.byref(d2), mid, wp2, s2, b2, y, capi.OUT_F32, ws, wsb), "conv2")
                ck(L.plhip_hard_act_f32(h, 1, sigm, y, gate, null, 1.0, n * c), "sigmoid")
            variants[tag + "/separate"] = sep
            variants[tag + "/se_gate"] = lambda gd=gd, pooled=pooled, gp=gp, s1=s1, b1=b1, s2=s2, b2=b2, gate=gate: ck(
                L.plhip_se_gate_int8(h, C.byref(gd), pooled, gp, s1, b1, s2, b2, gate), "se_gate")
        res = _alternate(ctx, variants, reps, inner)
        for k, b in nbytes.items():
            res[k]["algorithmic_bytes"] = b
            res[k]["tb_per_s"] = round(b / res[k]["median_us"] / 1e6, 3)
    return res


def networks(lite, wl, steps, batch):
    res = {}
    modes = {"unfused": dict(fuse=False), "fused_default": dict(fuse=True), "fused_j123": dict(fuse=True, fuse_hard_act=True)}
    for variant in ("large", "small"):
        net = wl.mobilenet_v3_net(variant)
        img = np.random.default_rng(5).uniform(-1, 1, (batch, 3, 224, 224)).astype(np.float32)
        preds = {}
        try:
            for m, kw in modes.items():
                p = lite.Predictor(0)
                preds[m] = p
                wl.emit_graph(p, net, batch, **kw)
                p.graph_lower()
                p.set_input(net["input"], img)
                p.run()
                for _ in range(3):  # warm-up
                    p.run(skip_io_copy=True)
                p.sync()
            t = {m: [] for m in modes}
            for _ in range(steps):
                for m, p in preds.items():
                    t0 = time.perf_counter()
                    p.run(skip_io_copy=True)
                    p.sync()
                    t[m].append(time.perf_counter() - t0)
            res[variant] = {m: dict(img_per_s=round(batch / statistics.median(v), 1), median_ms=round(statistics.median(v) * 1e3, 3),
                                    min_ms=round(min(v) * 1e3, 3), max_ms=round(max(v) * 1e3, 3), instructions=preds[m].num_instructions())
                            for m, v in t.items()}
        finally:
            for p in preds.values():
                p.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.import_package()
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    out = dict(tool="mbv3_bench", batch=a.batch, reps=a.reps, inner=a.inner, steps=a.steps, warmup="2 launches per kernel variant, 3 steps per program",
               rewrites=rewrites(pkg.capi, a.reps, a.inner), networks=networks(lite, wl, a.steps, a.batch))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
