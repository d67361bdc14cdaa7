#!/usr/bin/env python3
"""conv2d_transpose A/B through the C ABI (the method of DESIGN.md 11): one process, device-resident buffers, device
events on the context's stream, 5 warm-up calls of every candidate, then --rounds rounds in which the candidates of a shape alternate;
a window is as many calls as fill --window-ms (at least --reps; counted once per candidate from a trial window, then fixed), its time
elapsed / calls.  int8 output, relu, batch 32.

Candidates per shape:
  phase   plhip_conv2d_transpose_int8 on the MFMA phase route (where the shape is inside its envelope)
  direct  the same call with knob DECONV_ROUTE = 1: yardstick (a)
  conv    k 2 s 2 shapes only, yardstick (b): plhip_conv2d_int8 on the 1x1 conv Cin -> 4 Cout of the same plane: the same MACs, the
          same bytes in and out, without the pixel interleave
  conv2   the same 1x1 conv a second time in every round: the off-vs-off spread, yardstick (c)
Per shape the JSON records every window, the medians, the algorithmic bytes (input + output + filter) and MACs, achieved bytes/s
and int8 op/s, whether the phase route beat the direct route in every round by more than the spread of (c), and the ratio to (b).
Writes profiles/deconv.json (--out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

capi = ge.import_package().capi

# (name, cin, cout, h = w, k, stride, pad, groups)
SHAPES = [
    ("up_256_128_32_k2s2", 256, 128, 32, 2, 2, 0, 1),
    ("up_128_64_64_k2s2", 128, 64, 64, 2, 2, 0, 1),
    ("up_256_128_32_k4s2p1", 256, 128, 32, 4, 2, 1, 1),
    ("conv_64_64_64_k3s1p1", 64, 64, 64, 3, 1, 1, 1),
    ("dw_21_64_k4s2p1", 21, 21, 64, 4, 2, 1, 21),
]


def window(ctx, fn, reps):
    L = ctx.L
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.plhip_event_create(ctx.h, C.byref(e0))
    L.plhip_event_create(ctx.h, C.byref(e1))
    L.plhip_event_record(ctx.h, e0)
    for _ in range(reps):
        fn()
    L.plhip_event_record(ctx.h, e1)
    ctx.sync()
    ms = C.c_float()
    ctx.check(L.plhip_event_elapsed_ms(ctx.h, e0, e1, C.byref(ms)), "elapsed")
    L.plhip_event_destroy(ctx.h, e0)
    L.plhip_event_destroy(ctx.h, e1)
    return ms.value / reps


def bench_shape(ctx, rng, shape, batch, rounds, reps, warmup, window_ms):
    name, cin, cout, hw, k, s, p, g = shape
    L = ctx.L
    d = capi.deconv_desc(batch, cin, hw, hw, cout, k, k, (p, p, p, p), (s, s), (1, 1), g, capi.ACT_RELU, 0.0)
    oh, ow = capi.deconv_out_hw(d)
    w = rng.integers(-127, 128, (cin, cout // g, k, k), dtype=np.int8)
    dx, dw = ctx.to_device(rng.integers(-127, 128, (batch, cin, hw, hw), dtype=np.int8)), ctx.to_device(w)
    ds, db = ctx.to_device(np.full(cout, 1e-4, np.float32)), ctx.to_device(np.zeros(cout, np.float32))
    dy = ctx.malloc(batch * cout * oh * ow)
    cands = {}
    for knob, tag in ((0, "phase"), (1, "direct")):
        assert L.plhip_debug_set(b"DECONV_ROUTE", knob) == 0
        impl = capi.deconv_impl_name(d)
        if tag == "phase" and impl != "deconv_phase_int8_mfma32x32x32":
            continue  # outside the envelope: the direct route alone
        dwp = ctx.malloc(L.plhip_deconv_packed_weight_bytes(C.byref(d)))
        ctx.check(L.plhip_pack_deconv_weights(ctx.h, C.byref(d), dw, dwp), "pack")

        def run(knob=knob, dwp=dwp):
            L.plhip_debug_set(b"DECONV_ROUTE", knob)
            ctx.check(L.plhip_conv2d_transpose_int8(ctx.h, C.byref(d), dx, dwp, ds, db, dy, capi.OUT_I8), "conv2d_transpose")
        cands[tag] = (impl, run)
    L.plhip_debug_set(b"DECONV_ROUTE", 0)
    if k == 2 and s == 2 and p == 0 and g == 1:  # yardstick (b): the 1x1 conv with 4 Cout outputs on the same plane
        dc = capi.conv_desc(batch, cin, hw, hw, 4 * cout, 1, 1, act=capi.ACT_RELU)
        dwc = ctx.to_device(rng.integers(-127, 128, (4 * cout, cin, 1, 1), dtype=np.int8))
        dwcp = ctx.malloc(L.plhip_conv_packed_weight_bytes(C.byref(dc)))
        ctx.check(L.plhip_pack_conv_weights(ctx.h, C.byref(dc), dwc, dwcp), "pack")
        assert L.plhip_conv_workspace_bytes(C.byref(dc)) == 0
        ds4, dyc = ctx.to_device(np.full(4 * cout, 1e-4, np.float32)), ctx.malloc(batch * 4 * cout * hw * hw)

        def run_conv():
            ctx.check(L.plhip_conv2d_int8(ctx.h, C.byref(dc), dx, dwcp, ds4, None, dyc, capi.OUT_I8, None, 0), "conv2d")
        impl = L.plhip_conv_impl_name(C.byref(dc)).decode()
        cands["conv"] = (impl, run_conv)
        cands["conv2"] = (impl, run_conv)
    for _, run in cands.values():
        for _ in range(warmup):
            run()
    ctx.sync()
    calls = {tag: max(reps, min(4000, int(np.ceil(window_ms / max(window(ctx, run, reps), 1e-6))))) for tag, (_, run) in cands.items()}
    if "conv" in calls:
        calls["conv2"] = calls["conv"]
    ms = {tag: [] for tag in cands}
    for _ in range(rounds):
        for tag, (_, run) in cands.items():
            ms[tag].append(window(ctx, run, calls[tag]))
    taps = -(-k // s)
    rec = dict(name=name, batch=batch, cin=cin, cout=cout, h=hw, w=hw, k=k, stride=s, pad=p, groups=g, oh=oh, ow=ow,
               bytes=int(batch * (cin * hw * hw + cout * oh * ow) + w.size),
               # products the op needs: every input pixel meets every filter tap of its group's output channels
               macs=int(batch * hw * hw * cin * (cout // g) * k * k),
               impl={tag: impl for tag, (impl, _) in cands.items()}, calls_per_window=calls, windows_ms=ms,
               median_ms={tag: float(np.median(v)) for tag, v in ms.items()}, taps_per_output=taps * taps)
    for tag, t in rec["median_ms"].items():
        rec.setdefault("bytes_per_s", {})[tag] = rec["bytes"] / (t * 1e-3)
        rec.setdefault("int8_ops_per_s", {})[tag] = 2 * rec["macs"] / (t * 1e-3)
    if "conv" in ms:
        a, b = np.array(ms["conv"]), np.array(ms["conv2"])
        rec["spread_off_vs_off"] = float(np.max(np.abs(a - b) / np.minimum(a, b)))
        rec["phase_over_conv1x1"] = rec["median_ms"]["phase"] / rec["median_ms"]["conv"]
    if "phase" in ms:
        rec["direct_over_phase_per_round"] = [float(dv / pv) for dv, pv in zip(ms["direct"], ms["phase"])]
    ctx.free_all()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10, help="calls per window at least")
    ap.add_argument("--window-ms", type=float, default=5.0, help="a window holds as many calls as fill this time")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deconv.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    recs = []
    with capi.Context(0) as ctx:
        for shape in SHAPES:
            rec = bench_shape(ctx, rng, shape, args.batch, args.rounds, args.reps, args.warmup, args.window_ms)
            recs.append(rec)
            print("%-24s %s" % (rec["name"], "  ".join("%s %.1f us" % (t, v * 1e3) for t, v in rec["median_ms"].items())), flush=True)
    # the spread of yardstick (c), the largest over the shapes that have it, decides for every shape of this run
    spread = max([r["spread_off_vs_off"] for r in recs if "spread_off_vs_off" in r] or [0.0])
    for r in recs:
        if "direct_over_phase_per_round" in r:
            r["phase_beats_direct_every_round_by_more_than_spread"] = bool(min(r["direct_over_phase_per_round"]) > 1.0 + spread)
    out = dict(method="one process, device events, %d warm-up calls, %d rounds alternating the candidates, windows of >= %g ms and >= %d calls" % (
        args.warmup, args.rounds, args.window_ms, args.reps), batch=args.batch, spread_off_vs_off=spread, shapes=recs)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("spread %.4f -> %s" % (spread, args.out))


if __name__ == "__main__":
    main()
