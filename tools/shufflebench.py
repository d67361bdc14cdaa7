"""ShuffleNetV2 on the device: what fusion K costs and saves.  One process, the variants alternated in one loop,
device events around whole steps on the predictors' stream, warm-up stated.  Prints one JSON line and writes it to --out.

(a) ShuffleNetV2 1.0, batch 128, 224 x 224, one step in flight (run(skip_io_copy=True), resident input): the default fusions with K
    off and with K on, alternating; --steps rounds after --warmup steps each.  The K-off program is timed TWICE per round (off_a,
    off_b): the spread between two runs of the same program is what a difference between K off and K on has to beat.
(b) --kernels: the unit tail at the three stage shapes of that network (h x plane: 58 x 784, 116 x 196, 232 x 49; batch 128), one
    launch of plhip_shuffle_unit_f32 against the four launches it replaces, and plhip_calib_f32_to_i8 moving the same number of
    bytes (13 h P per image: a plain stream of the same size), --inner launches between two events.  Run this part under
    `rocprofv3 --kernel-trace --stats` for per-kernel times; the events here time launch sequences.

    python tools/shufflebench.py [--steps 20] [--warmup 5] [--batch 128] [--kernels] [--out profiles/shufflenet_k.json]
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

STAGE_SHAPES = ((58, 784), (116, 196), (232, 49))  # half width, plane of the stride-1 units of ShuffleNetV2 1.0


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
    net = wl.shufflenet_v2_net(1.0)
    img = np.random.default_rng(5).uniform(-1, 1, (batch, 3, 224, 224)).astype(np.float32)
    modes = {"k_off_a": dict(fuse=True, fuse_shuffle=False), "k_on": dict(fuse=True, fuse_shuffle=True), "k_off_b": dict(fuse=True, fuse_shuffle=False)}
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
            ref = preds["k_off_a"].get_var(out_name, np.float32)
            same = bool(np.array_equal(ref.view(np.uint32), preds["k_on"].get_var(out_name, np.float32).view(np.uint32)))
            t = {m: [] for m in modes}
            for _ in range(steps):
                for m, p in preds.items():
                    t[m].append(_timed_ms(ctx, ev, lambda p=p: p.run(skip_io_copy=True)))
            res = {m: dict(_stat(v), img_per_s=round(batch / statistics.median(v) * 1e3, 1), instructions=preds[m].num_instructions())
                   for m, v in t.items()}
        finally:
            for p in preds.values():
                p.close()
    off_a, off_b, on = (res[k]["median_ms"] for k in ("k_off_a", "k_off_b", "k_on"))
    # per-round differences: the same program against itself (the spread) and K on against the mean of the two K-off runs
    self_diff = [abs(a - b) for a, b in zip(t["k_off_a"], t["k_off_b"])]
    gain = [(a + b) / 2 - o for a, b, o in zip(t["k_off_a"], t["k_off_b"], t["k_on"])]
    res["k_off_spread_ms"] = dict(median_abs_diff=round(statistics.median(self_diff), 4), max_abs_diff=round(max(self_diff), 4),
                                  medians_diff=round(abs(off_a - off_b), 4))
    res["k_on_gain_ms"] = dict(median=round(statistics.median(gain), 4), min=round(min(gain), 4), max=round(max(gain), 4))
    res["k_on_beats_spread"] = bool(statistics.median(gain) > max(statistics.median(self_diff), abs(off_a - off_b)) and min(gain) > 0)
    res["outputs_bit_identical"] = same
    sep, fused = wl.shuffle_unit_bytes(net, batch)
    res["unit_tail_bytes_per_step"] = dict(separate=sep, fused=fused)
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
        for hc, hw in STAGE_SHAPES:
            tag = "h%d_p%d" % (hc, hw)
            cnt = batch * hc * hw  # elements of one operand
            a = ctx.to_device((rng.standard_normal(cnt) * 2).astype(np.float32))
            b = ctx.to_device((rng.standard_normal(cnt) * 2).astype(np.float32))
            cat, shuf = ctx.malloc(8 * cnt), ctx.malloc(8 * cnt)
            lo, hi, q = ctx.malloc(4 * cnt), ctx.malloc(4 * cnt), ctx.malloc(cnt)
            two = (C.c_void_p * 2)(a, b)
            outs = (C.c_void_p * 2)(lo, hi)
            ext = (C.c_int64 * 2)(hc, hc)

            def sep(two=two, ext=ext, cat=cat, shuf=shuf, outs=outs, hi=hi, q=q, hc=hc, hw=hw, cnt=cnt):
                ck(L.plhip_concat_f32(h, two, ext, 2, batch, hw, cat), "concat")
                ck(L.plhip_shuffle_channel_f32(h, cat, batch, 2 * hc, hw, 2, shuf, null, 1.0), "shuffle")
                ck(L.plhip_split_f32(h, shuf, batch, 2 * hc, hw, 2, None, 2, outs), "split")
                ck(L.plhip_calib_f32_to_i8(h, hi, q, scale, cnt), "calib")
            variants[tag + "/separate"] = sep
            variants[tag + "/unit"] = lambda a=a, b=b, lo=lo, q=q, hc=hc, hw=hw: ck(
                L.plhip_shuffle_unit_f32(h, a, b, batch, hc, hw, hc, lo, null, q, scale), "unit")
            # a plain stream of the unit's 13 h P bytes: calib reads 4 and writes 1 byte per element, so 13 / 5 elements per h P
            n_stream = cnt * 13 // 5
            sx, sq = ctx.malloc(4 * n_stream), ctx.malloc(n_stream)
            ck(L.plhip_memset(h, sx, 0, 4 * n_stream), "memset")
            variants[tag + "/calib_same_bytes"] = lambda sx=sx, sq=sq, n_stream=n_stream: ck(L.plhip_calib_f32_to_i8(h, sx, sq, scale, n_stream), "calib")
            nbytes[tag + "/separate"] = 53 * cnt
            nbytes[tag + "/unit"] = 13 * cnt
            nbytes[tag + "/calib_same_bytes"] = 5 * n_stream
        for fn in variants.values():
            fn(), fn()
        ctx.sync()
        t = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                t[k].append(_timed_ms(ctx, ev, fn, inner) * 1e3)
        for k, v in t.items():
            res[k] = dict(_stat(v, "us", 3), algorithmic_bytes=nbytes[k], tb_per_s=round(nbytes[k] / statistics.median(v) / 1e6, 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--kernels", action="store_true", help="also time the unit kernel against the launches it replaces")
    ap.add_argument("--kernels-only", action="store_true", help="part (b) alone (the run to put under rocprofv3)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.import_package()
    lite = importlib.import_module("paddle_lite_amd.liteapi")
    wl = importlib.import_module("paddle_lite_amd.workloads")
    out = dict(tool="shufflebench", model="shufflenet_v2 1.0", batch=a.batch, res=224, steps=a.steps,
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
