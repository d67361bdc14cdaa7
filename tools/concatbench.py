"""SqueezeNet v1.1 on the device: what fusion L costs and saves.  One process, the variants alternated in one loop,
device events around whole steps on the predictors' stream, warm-up stated.  Prints one JSON line and writes it to --out.

(a) SqueezeNet v1.1, batch 128, 224 x 224, one step in flight (run(skip_io_copy=True), resident input): the default fusions with L
    off and with L on, alternating; --steps rounds after --warmup steps each.  The L-off program is timed TWICE per round (off_a,
    off_b): the spread between two runs of the same program is what a difference between L off and L on has to beat.
(b) --kernels: plhip_concat_calib_f32 at the four concat shapes of that network (two operands of c x plane: 64 x 3025, 128 x 729,
    192 x 169, 256 x 169; batch 128), int8 output only (what L makes of every concat of the network), against the two launches it
    replaces (plhip_concat_f32, plhip_calib_f32_to_i8) and against plhip_calib_f32_to_i8 moving the same number of bytes (5 per
    concatenated element: a plain stream of the same size), --inner launches between two events.  Run this part under
    `rocprofv3 --kernel-trace --stats` for per-kernel times; the events here time launch sequences.

    python tools/concatbench.py [--steps 20] [--warmup 5] [--batch 128] [--kernels] [--out profiles/squeezenet_l.json]
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

CONCAT_SHAPES = ((64, 3025), (128, 729), (192, 169), (256, 169))  # channels of either operand, plane: fire2/3, 4/5, 6/7, 8/9


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


def network(capi, lite, wl, batch, steps, warmup):
    net = wl.squeezenet_v1_1_net()
    img = np.random.default_rng(5).uniform(-1, 1, (batch, 3, 224, 224)).astype(np.float32)
    modes = {"l_off_a": dict(fuse=True, fuse_concat=False), "l_on": dict(fuse=True, fuse_concat=True), "l_off_b": dict(fuse=True, fuse_concat=False)}
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
            out_name = net["output"]
            ref = preds["l_off_a"].get_var(out_name, np.float32)
            same = bool(np.array_equal(ref.view(np.uint32), preds["l_on"].get_var(out_name, np.float32).view(np.uint32)))
            t = {m: [] for m in modes}
            for _ in range(steps):
                for m, p in preds.items():
                    t[m].append(_timed_ms(ctx, ev, lambda p=p: p.run(skip_io_copy=True)))
            res = {m: dict(_stat(v), img_per_s=round(batch / statistics.median(v) * 1e3, 1), instructions=preds[m].num_instructions())
                   for m, v in t.items()}
        finally:
            for p in preds.values():
                p.close()
    off_a, off_b = res["l_off_a"]["median_ms"], res["l_off_b"]["median_ms"]
    # per-round differences: the same program against itself (the spread) and L on against the mean of the two L-off runs
    self_diff = [abs(a - b) for a, b in zip(t["l_off_a"], t["l_off_b"])]
    gain = [(a + b) / 2 - o for a, b, o in zip(t["l_off_a"], t["l_off_b"], t["l_on"])]
    res["l_off_spread_ms"] = dict(median_abs_diff=round(statistics.median(self_diff), 4), max_abs_diff=round(max(self_diff), 4),
                                  medians_diff=round(abs(off_a - off_b), 4))
    res["l_on_gain_ms"] = dict(median=round(statistics.median(gain), 4), min=round(min(gain), 4), max=round(max(gain), 4))
    res["l_on_beats_spread"] = bool(statistics.median(gain) > max(statistics.median(self_diff), abs(off_a - off_b)) and min(gain) > 0)
    res["outputs_bit_identical"] = same
    sep, fused = wl.concat_calib_bytes(net, batch)
    res["concat_calib_bytes_per_step"] = dict(separate=sep, fused=fused)
    return res


def kernels(capi, batch, reps, inner):
    rng = np.random.default_rng(11)
    res = {}
    with capi.Context(0) as ctx:
        L, h, ck = ctx.L, ctx.h, ctx.check
        ev = _events(ctx)
        null = C.c_void_p()
        scale = 4.0 / 127
        variants, nbytes = {}, {}
        for c, hw in CONCAT_SHAPES:
            tag = "c%d_p%d" % (c, hw)
            cnt = batch * c * hw  # elements of one operand
            a = ctx.to_device((rng.standard_normal(cnt) * 2).astype(np.float32))
            b = ctx.to_device((rng.standard_normal(cnt) * 2).astype(np.float32))
            cat, q = ctx.malloc(8 * cnt), ctx.malloc(2 * cnt)
            two = (C.c_void_p * 2)(a, b)
            ext = (C.c_int64 * 2)(c, c)

            def sep(two=two, ext=ext, cat=cat, q=q, hw=hw, cnt=cnt):
                ck(L.plhip_concat_f32(h, two, ext, 2, batch, hw, cat), "concat")
                ck(L.plhip_calib_f32_to_i8(h, cat, q, scale, 2 * cnt), "calib")
            variants[tag + "/separate"] = sep
            variants[tag + "/concat_calib"] = lambda two=two, ext=ext, q=q, hw=hw: ck(
                L.plhip_concat_calib_f32(h, two, ext, 2, batch, hw, null, q, scale), "concat_calib")
            # a plain stream of the same bytes: calib reads 4 and writes 1 byte per element, as the fused launch does
            variants[tag + "/calib_same_bytes"] = lambda cat=cat, q=q, cnt=cnt: ck(L.plhip_calib_f32_to_i8(h, cat, q, scale, 2 * cnt), "calib")
            nbytes[tag + "/separate"] = 13 * 2 * cnt
            nbytes[tag + "/concat_calib"] = 5 * 2 * cnt
            nbytes[tag + "/calib_same_bytes"] = 5 * 2 * cnt
        for fn in variants.values():
            fn(), fn()
        ctx.sync()
        t = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                t[k].append(_timed_ms(ctx, ev, fn, inner) * 1e3)
        for k, v in t.items():
            res[k] = dict(_stat(v, "us", 3), algorithmic_bytes=nbytes[k], tb_per_s=round(nbytes[k] / statistics.median(v) / 1e6, 3))
        for c, hw in CONCAT_SHAPES:
            tag = "c%d_p%d" % (c, hw)
            one, stream_, two_ = (res[tag + k]["median_us"] for k in ("/concat_calib", "/calib_same_bytes", "/separate"))
            res[tag + "/summary"] = dict(behind_plain_stream_pct=round(100 * (one / stream_ - 1), 1), of_the_two_launches_pct=round(100 * one / two_, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--kernels", action="store_true", help="also time the kernel against the launches it replaces")
    ap.add_argument("--kernels-only", action="store_true", help="part (b) alone (the run to put under rocprofv3)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.import_package()
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    out = dict(tool="concatbench", model="squeezenet_v1_1", batch=a.batch, res=224, steps=a.steps,
               warmup="%d steps per program; 2 launches per kernel variant" % a.warmup)
    if not a.kernels_only:
        out["network"] = network(pkg.capi, lite, wl, a.batch, a.steps, a.warmup)
    if a.kernels or a.kernels_only:
        out["kernels"] = kernels(pkg.capi, a.batch, a.reps, a.inner)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
