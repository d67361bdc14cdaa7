"""Dense prediction on the device: what the interp / arg_max kernels cost and what fusions M and N save.  One
process, the variants alternated in one loop, device events on one stream, warm-up stated.  Prints one JSON line and writes it
to --out.

(a) seg_mini_net, batch 32, 512 x 512, one step in flight (run(skip_io_copy=True), resident input): the default fusions with M and
    N off, M on, N on, both on, alternating; --steps rounds after --warmup steps each.  The off program is timed TWICE per round
    (off_a, off_b): the spread between two runs of the same program is what a difference has to beat.
(b) --kernels: the three entry points at a segmentation head (19 and 21 classes, 128 x 256 -> 512 x 1024, batch 8, bilinear with
    aligned corners) and a decoder stage (256 channels, 32 x 32 -> 128 x 128, batch 32, bilinear mode 1 and nearest):
      plhip_interp_f32 (fp32 out)   against plhip_calib_i8_to_f32 writing as many elements (a stream that writes 4 bytes per
                                    element and reads 1)
      plhip_interp_f32 (int8 only)  against plhip_interp_f32 (fp32) + plhip_calib_f32_to_i8
      plhip_interp_argmax_f32       against plhip_interp_f32 (fp32) + plhip_arg_max_f32          (the heads)
    --inner launches between two events.  Run this part under `rocprofv3 --kernel-trace --stats` for per-kernel times; the events
    here time launch sequences.

    python tools/interpbench.py [--steps 20] [--warmup 5] [--batch 32] [--res 512] [--kernels] [--out profiles/segnet_mn.json]
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

# (tag, n, c, in_h, in_w, out_h, out_w, method, align_corners, align_mode, with the arg_max comparison)
KERNEL_SHAPES = (("head19", 8, 19, 128, 256, 512, 1024, 0, 1, 1, True), ("head21", 8, 21, 128, 256, 512, 1024, 0, 1, 1, True),
                 ("decoder_bilinear", 32, 256, 32, 32, 128, 128, 0, 0, 1, False), ("decoder_nearest", 32, 256, 32, 32, 128, 128, 1, 0, 1, False))


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
    net = wl.seg_mini_net(res=res_px)
    img = np.random.default_rng(5).uniform(-1, 1, (batch, 3, res_px, res_px)).astype(np.float32)
    sw = lambda m, n: dict(fuse=True, fuse_interp_argmax=m, fuse_interp_calib=n)
    modes = {"off_a": sw(False, False), "m_on": sw(True, False), "n_on": sw(False, True), "mn_on": sw(True, True), "off_b": sw(False, False)}
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
            ref = preds["off_a"].get_var(net["output"], np.int64)
            same = all(bool(np.array_equal(ref, preds[m].get_var(net["output"], np.int64))) for m in ("m_on", "n_on", "mn_on"))
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
    # per-round differences: the same program against itself (the spread) and a fusion against the mean of the two off runs
    self_diff = [abs(a - b) for a, b in zip(t["off_a"], t["off_b"])]
    spread = max(statistics.median(self_diff), abs(off_a - off_b))
    res["off_spread_ms"] = dict(median_abs_diff=round(statistics.median(self_diff), 4), max_abs_diff=round(max(self_diff), 4),
                                medians_diff=round(abs(off_a - off_b), 4))
    for m in ("m_on", "n_on", "mn_on"):
        gain = [(a + b) / 2 - o for a, b, o in zip(t["off_a"], t["off_b"], t[m])]
        res[m + "_gain_ms"] = dict(median=round(statistics.median(gain), 4), min=round(min(gain), 4), max=round(max(gain), 4))
        res[m + "_beats_spread"] = bool(statistics.median(gain) > spread and min(gain) > 0)
    res["labels_identical"] = same
    return res


def kernels(capi, reps, inner):
    rng = np.random.default_rng(11)
    res = {}
    with capi.Context(0) as ctx:
        L, h, ck = ctx.L, ctx.h, ctx.check
        ev = _events(ctx)
        null = C.c_void_p()
        scale = 4.0 / 127
        for tag, n, c, ih, iw, oh, ow, method, ac, am, with_argmax in KERNEL_SHAPES:
            planes, cnt_in, cnt = n * c, n * c * ih * iw, n * c * oh * ow
            x = ctx.to_device((rng.standard_normal(cnt_in) * 2).astype(np.float32))
            yf, yq, lab = ctx.malloc(4 * cnt), ctx.malloc(cnt), ctx.malloc(8 * n * oh * ow)
            ck(L.plhip_memset(h, yq, 1, cnt), "memset")
            args = (ih, iw, oh, ow, method, ac, am)
            variants, nbytes = {}, {}
            variants["interp_f32"] = lambda: ck(L.plhip_interp_f32(h, x, planes, *args, yf, null, 1.0), "interp")
            variants["stream_i8_to_f32"] = lambda: ck(L.plhip_calib_i8_to_f32(h, yq, yf, scale, cnt), "calib")
            variants["interp_i8"] = lambda: ck(L.plhip_interp_f32(h, x, planes, *args, null, yq, scale), "interp")

            def two_calib():
                ck(L.plhip_interp_f32(h, x, planes, *args, yf, null, 1.0), "interp")
                ck(L.plhip_calib_f32_to_i8(h, yf, yq, scale, cnt), "calib")
            variants["interp_f32+calib"] = two_calib
            nbytes.update({"interp_f32": 4 * cnt_in + 4 * cnt, "stream_i8_to_f32": 5 * cnt, "interp_i8": 4 * cnt_in + cnt,
                           "interp_f32+calib": 4 * cnt_in + 9 * cnt})
            if with_argmax:
                variants["interp_argmax"] = lambda: ck(L.plhip_interp_argmax_f32(h, x, n, c, *args, lab, -1), "interp_argmax")

                def two_argmax():
                    ck(L.plhip_interp_f32(h, x, planes, *args, yf, null, 1.0), "interp")
                    ck(L.plhip_arg_max_f32(h, yf, n, c, oh * ow, lab, -1), "arg_max")
                variants["interp_f32+arg_max"] = two_argmax
                nbytes.update({"interp_argmax": 4 * cnt_in + 8 * n * oh * ow, "interp_f32+arg_max": 4 * cnt_in + 8 * cnt + 8 * n * oh * ow})
            for fn in variants.values():
                fn(), fn()
            ctx.sync()
            t = {k: [] for k in variants}
            for _ in range(reps):
                for k, fn in variants.items():
                    t[k].append(_timed_ms(ctx, ev, fn, inner) * 1e3)
            r = {k: dict(_stat(v, "us", 3), algorithmic_bytes=nbytes[k], tb_per_s=round(nbytes[k] / statistics.median(v) / 1e6, 3)) for k, v in t.items()}
            med = lambda k: r[k]["median_us"]
            r["summary"] = dict(interp_f32_over_stream=round(med("interp_f32") / med("stream_i8_to_f32"), 3),
                                interp_i8_over_two_launches=round(med("interp_i8") / med("interp_f32+calib"), 3))
            if with_argmax:
                r["summary"]["interp_argmax_over_two_launches"] = round(med("interp_argmax") / med("interp_f32+arg_max"), 3)
            res[tag] = r
            for p in (x, yf, yq, lab):
                ctx.free(p)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--kernels", action="store_true", help="also time the kernels against their yardsticks")
    ap.add_argument("--kernels-only", action="store_true", help="part (b) alone (the run to put under rocprofv3)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.import_package()
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    out = dict(tool="interpbench", model="seg_mini", batch=a.batch, res=a.res, steps=a.steps,
               warmup="%d steps per program; 2 launches per kernel variant" % a.warmup)
    if not a.kernels_only:
        out["network"] = network(pkg.capi, lite, wl, a.batch, a.res, a.steps, a.warmup)
    if a.kernels or a.kernels_only:
        out["kernels"] = kernels(pkg.capi, a.reps, a.inner)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
