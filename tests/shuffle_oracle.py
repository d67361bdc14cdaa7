"""CPU oracle for op-list networks that use the three fp32 ops ShuffleNetV2 adds (paddle-lite_amd/workloads.py
shufflenet_v2_net).  TEST INFRASTRUCTURE, next to mbv3_oracle.py.

The ops move values; they are restated in numpy index arithmetic from the reference's loops (no value is recomputed, so NaN
payloads and -0.0 keep their bits):
  concat           lite/kernels/arm/concat_compute.cc:37-57 (ConcatFunc): input i's rows of c_i * inner elements are copied behind
                   one another into rows of sum(c_i) * inner elements, `outer` times
  split            lite/backends/arm/math/split.cc:54-82: output i takes `out_after` = c_i * inner elements of every row of
                   `in_after` = C * inner elements, starting where output i - 1 ended; extents from num (equal parts) or
                   sections (lite/operators/split_op.cc:32-75)
  shuffle_channel  lite/backends/arm/math/shuffle_channel.cc:24-55: per image, plane i * group_col + j goes to plane
                   j * group_row + i, group_row = group, group_col = C / group
plan() restates oracle/graph_oracle.py's plan rule (static_kernel_pick_pass.cc:92-165, type_precision_cast_pass.cc:60-100)
with the three ops as fp32 ops like pool2d, N inputs for concat and one entry per output for split; forward() calls oracle/plref
for everything graph_oracle.forward computes."""
import numpy as np

INT8_OPS = ("conv2d", "depthwise_conv2d", "fc")
F32 = np.float32


def _axis_split(shape, axis):
    axis = axis + len(shape) if axis < 0 else axis
    assert 0 <= axis < len(shape)
    return axis, int(np.prod(shape[:axis], dtype=np.int64)), int(np.prod(shape[axis + 1:], dtype=np.int64))


def concat(xs, axis):
    """concat_compute.cc:37-57 as loops over rows: out[o][off_i : off_i + len_i] = x_i[o][:]."""
    xs = [np.ascontiguousarray(x) for x in xs]
    axis, outer, inner = _axis_split(xs[0].shape, axis)
    for x in xs[1:]:
        assert x.shape[:axis] == xs[0].shape[:axis] and x.shape[axis + 1:] == xs[0].shape[axis + 1:]
    lens = [x.shape[axis] * inner for x in xs]
    out = np.empty((outer, sum(lens)), xs[0].dtype)
    off = 0
    for x, n in zip(xs, lens):
        flat = x.reshape(outer, n)
        for o in range(outer):
            out[o, off:off + n] = flat[o]
        off += n
    shape = list(xs[0].shape)
    shape[axis] = sum(x.shape[axis] for x in xs)
    return out.reshape(shape)


def split_extents(extent, count, num=0, sections=()):
    """split_op.cc:32-75: num > 0 equal parts, else the sections."""
    if num > 0:
        assert count == num and extent % num == 0
        return [extent // num] * num
    assert len(sections) == count and sum(sections) == extent
    return list(sections)


def split(x, axis, num=0, sections=(), count=None):
    """split.cc:54-82: for each output, `before` copies of out_after elements with the input stepping in_after."""
    x = np.ascontiguousarray(x)
    axis, outer, inner = _axis_split(x.shape, axis)
    ext = split_extents(x.shape[axis], count if count is not None else (num if num > 0 else len(sections)), num, sections)
    flat = x.reshape(outer, x.shape[axis] * inner)
    outs, off = [], 0
    for e in ext:
        part = np.empty((outer, e * inner), x.dtype)
        for o in range(outer):
            part[o] = flat[o, off:off + e * inner]
        off += e * inner
        shape = list(x.shape)
        shape[axis] = e
        outs.append(part.reshape(shape))
    return outs


def shuffle_channel(x, group):
    """shuffle_channel.cc:24-55: out[b][j * group + i] = in[b][i * (c / group) + j]."""
    x = np.ascontiguousarray(x)
    n, c = x.shape[:2]
    assert c % group == 0
    cols = c // group
    src = x.reshape(n, c, -1)
    out = np.empty_like(src)
    for i in range(group):
        for j in range(cols):
            out[:, j * group + i] = src[:, i * cols + j]
    return out.reshape(x.shape)


def calib_i8(y, scale):
    """calib[fp32_to_int8] (type_trans.cc:45, 183-184): round half away from zero of y * (1.f / scale), clamped to +-127;
    NaN becomes 0 as the device's float -> int conversion makes it."""
    inv = F32(1.0) / F32(scale)
    with np.errstate(all="ignore"):
        v = (np.asarray(y, F32) * inv).astype(F32)
        v = np.where(np.isnan(v), F32(0), np.clip(v, F32(-127), F32(127)))
        return (np.sign(v) * np.floor(np.abs(v).astype(np.float64) + 0.5)).astype(np.int8)


def shuffle_unit(a, b, split_at, calib_scale=None):
    """The composition the fused tail replaces: concat([a, b], 1) -> shuffle_channel(2) -> split at split_at -> calib of the second
    part.  Returns (lo, hi, hi_i8 or None)."""
    s = shuffle_channel(concat([a, b], 1), 2)
    c = s.shape[1]
    lo, hi = split(s, 1, sections=(split_at, c - split_at)) if 0 < split_at < c else ((s[:, :0], s) if split_at == 0 else (s, s[:, :0]))
    return lo, hi, (calib_i8(hi, calib_scale) if calib_scale is not None else None)


def ins_of(o):
    t = o["op"]
    if t in ("add", "mul"):
        return [o["x"], o["y"]]
    if t == "concat":
        return list(o["srcs"])
    return [o["src"]]


def outs_of(o):
    return list(o["names"]) if o["op"] == "split" else [o["name"]]


def plan(net):
    """[(kind, dict)] in execution order; kind in {calib, op}."""
    ops = net["ops"]
    consumers = {}
    for i, o in enumerate(ops):
        for v in ins_of(o):
            consumers.setdefault(v, []).append(i)
    steps, prec, cast = [], {net["input"]: "f32"}, {}
    for o in ops:
        is8 = o["op"] in INT8_OPS
        want = "i8" if is8 else "f32"
        use = []
        for v in ins_of(o):
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
        for v in outs_of(o):
            prec[v] = "i8" if int8_out else "f32"
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
            x = T[ins[0]]
            if o["global_pooling"] and o["pooling_type"] == "avg":
                put(o["name"], plref.global_avg_pool(x))
            else:
                p = o["pad"]
                put(o["name"], plref.pool2d(x, o["pooling_type"], (o["ksize"],) * 2, (o["stride"],) * 2, (p, p, p, p), exclusive=True,
                                            ceil_mode=False))
        elif t == "add":
            put(o["name"], plref.elementwise_add(T[ins[0]], T[ins[1]], o["act"] == "relu"))
        elif t == "softmax":
            put(o["name"], plref.softmax(T[ins[0]]))
        elif t == "concat":
            put(o["name"], concat([T[v] for v in ins], o["axis"]))
        elif t == "split":
            for name, part in zip(o["names"], split(T[ins[0]], o["axis"], o["num"], o["sections"], count=len(o["names"]))):
                put(name, part)
        elif t == "shuffle_channel":
            put(o["name"], shuffle_channel(T[ins[0]], o["group"]))
        else:
            raise ValueError(t)
    return out
