"""CPU oracle for op-list networks that use the three fp32 ops MobileNetV3 adds (paddle-lite_amd/workloads.py
mobilenet_v3_net).  TEST INFRASTRUCTURE, next to mbv1_oracle.py.

The ops are restated in numpy float32 from the reference's scalar C (every operation below is one IEEE fp32 operation, so
the restatement is exact, NaN and infinities included):
  hard_swish    lite/backends/arm/math/activation.cc:716-731   min(max(0.f, x + offset), threshold) * x / scale, left to
                right; std::max(0.f, v) is `0.f < v ? v : 0.f`, std::min(a, t) is `t < a ? t : a`; defaults threshold 6,
                scale 6, offset 3 (lite/operators/op_params.h:409-412)
  hard_sigmoid  activation.cc:678-691   t = x * slope + offset (a multiply and an add, two roundings);
                t = t < 1 ? t : 1; t = t > 0 ? t : 0; defaults slope 0.2, offset 0.5 (op_params.h:406-408)
  mul           lite/kernels/arm/elementwise_compute.cc:30-84, fast broadcast pre = 1, n = N * C, post = H * W:
                out[n][c][i] = x[n][c][i] * y[n][c]
plan() restates oracle/graph_oracle.py's plan rule (static_kernel_pick_pass.cc:92-165, type_precision_cast_pass.cc:60-100)
with the three ops as fp32 ops like pool2d and add; forward() calls oracle/plref for everything graph_oracle.forward
computes."""
import numpy as np

INT8_OPS = ("conv2d", "depthwise_conv2d", "fc")
F32 = np.float32


def hard_swish(x, threshold=6.0, scale=6.0, offset=3.0):
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        t = x + F32(offset)
        t = np.where(F32(0) < t, t, F32(0)).astype(F32)
        t = np.where(F32(threshold) < t, F32(threshold), t).astype(F32)
        return ((t * x).astype(F32) / F32(scale)).astype(F32)


def hard_sigmoid(x, slope=0.2, offset=0.5):
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        t = ((x * F32(slope)).astype(F32) + F32(offset)).astype(F32)
        t = np.where(t < F32(1), t, F32(1)).astype(F32)
        return np.where(t > F32(0), t, F32(0)).astype(F32)


def se_scale(x, gate):
    x = np.asarray(x, F32)
    g = np.asarray(gate, F32).reshape(x.shape[0], x.shape[1], *([1] * (x.ndim - 2)))
    with np.errstate(all="ignore"):
        return (x * g).astype(F32)


def calib_i8(y, scale):
    """calib[fp32_to_int8] (type_trans.cc:45, 183-184): round half away from zero of y * (1.f / scale), clamped to +-127;
    NaN becomes 0 as the device's float -> int conversion makes it."""
    inv = F32(1.0) / F32(scale)
    with np.errstate(all="ignore"):
        v = (np.asarray(y, F32) * inv).astype(F32)
        v = np.where(np.isnan(v), F32(0), np.clip(v, F32(-127), F32(127)))
        return (np.sign(v) * np.floor(np.abs(v).astype(np.float64) + 0.5)).astype(np.int8)


def _ins(o):
    return [o["x"], o["y"]] if o["op"] in ("add", "mul") else [o["src"]]


def plan(net):
    """[(kind, dict)] in execution order; kind in {calib, op}."""
    ops = net["ops"]
    consumers = {}
    for i, o in enumerate(ops):
        for v in _ins(o):
            consumers.setdefault(v, []).append(i)
    steps, prec, cast = [], {net["input"]: "f32"}, {}
    for o in ops:
        is8 = o["op"] in INT8_OPS
        want = "i8" if is8 else "f32"
        use = []
        for v in _ins(o):
            if prec[v] != want:
                if v not in cast:
                    assert want == "i8", "int8 -> fp32 casts do not occur in these graphs"
                    cast[v] = v + "/precision_trans"
                    steps.append(("calib", dict(src=v, dst=cast[v], scale=float(o["in_scale"]))))
                use.append(cast[v])
            else:
                use.append(v)
        int8_out, oscale = False, 1.0
        if is8:
            cs = consumers.get(o["name"], [])
            int8_out = bool(cs) and all(ops[c]["op"] in INT8_OPS for c in cs) and o["name"] != net["output"]
            if int8_out:
                oscale = float(ops[cs[0]]["in_scale"])
        steps.append(("op", dict(o=o, ins=use, int8_out=int8_out, oscale=oscale)))
        prec[o["name"]] = "i8" if int8_out else "f32"
    return steps


def forward(plref, net, image, via_gemm=False):
    """name -> tensor for every variable of the unfused lowered program ("<var>/precision_trans" for calib outputs)."""
    T = {net["input"]: np.ascontiguousarray(image, F32)}
    out = {}

    def put(name, val):
        T[name] = out[name] = val

    for kind, s in plan(net):
        if kind == "calib":
            put(s["dst"], plref.calib_f32_to_i8(T[s["src"]], s["scale"]))
            continue
        o, ins = s["o"], s["ins"]
        t = o["op"]
        if t in ("conv2d", "depthwise_conv2d"):
            x = T[ins[0]]
            cout, cg, k, _ = o["w"].shape
            p = o["pad"]
            sh = plref.shape(x.shape[0], x.shape[1], x.shape[2], x.shape[3], cout, k, k, (p, p, p, p), (o["stride"],) * 2, (1, 1),
                             o["groups"])
            y, _ = plref.conv2d(sh, x, o["w"], o["bias"], float(o["in_scale"]), o["w_scale"], s["oscale"], o["act"], o["act_coef"],
                                s["int8_out"], via_gemm=(via_gemm and o["groups"] == 1))
            put(o["name"], y)
        elif t == "fc":
            x = T[ins[0]]
            x2 = x.reshape(x.shape[0], -1)
            assert not s["int8_out"]
            sc = (o["w_scale"] * F32(o["in_scale"])).astype(F32)
            y, _ = plref.fc(x2, o["w"], o["bias"], sc, False, False, route=plref.fc_route(x2.shape[0], o["w_scale"].size))
            put(o["name"], y)
        elif t == "pool2d":
            assert o["global_pooling"] and o["pooling_type"] == "avg"
            put(o["name"], plref.global_avg_pool(T[ins[0]]))
        elif t == "add":
            put(o["name"], plref.elementwise_add(T[ins[0]], T[ins[1]], o["act"] == "relu"))
        elif t == "softmax":
            put(o["name"], plref.softmax(T[ins[0]]))
        elif t == "hard_swish":
            put(o["name"], hard_swish(T[ins[0]]))
        elif t == "hard_sigmoid":
            put(o["name"], hard_sigmoid(T[ins[0]]))
        elif t == "mul":
            put(o["name"], se_scale(T[ins[0]], T[ins[1]]))
        else:
            raise ValueError(t)
    return out
