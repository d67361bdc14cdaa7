"""conv2d_transpose on int8, stated once in numpy: the semantics plhip_conv2d_transpose_int8 is held to.

x int8 [N, Cin, H, W]; filter int8 [Cin, Cout / groups, kh, kw] (the reference's "chin * chout * kh * kw", no flip); paddings
(top, bottom, left, right); strides and dilations (h, w).  OH = (H - 1) sh - pt - pb + dh (kh - 1) + 1 (the width alike); an
output_size entry o with OH <= o < OH + sh replaces OH, anything else is an error.  int32 accumulator

    acc[n, g Mg + m, iy sh - pt + r dh, ix sw - pl + s dw] += x[n, g Cg + c, iy, ix] * w[g Cg + c, m, r, s]

with targets outside the output dropped; outputs no tap reaches are 0.  The epilogue is conv's (plref.epilogue on the
accumulators, scales folded by plref.fold_scales).  Two forms of the accumulator: `acc_scatter` is the sentence above, one
shifted slice per tap; `acc_gather` is the form the kernels use, per output row / column and tap the input index
iy = (oy + pt - r dh) / sh where that divides and is in range."""
import numpy as np


def out_dims(h, w, kh, kw, pads, strides, dils, output_size=(0, 0)):
    """(OH, OW); ValueError for a non-positive default or an output_size entry outside [default, default + stride)."""
    dflt = ((h - 1) * strides[0] - pads[0] - pads[1] + dils[0] * (kh - 1) + 1,
            (w - 1) * strides[1] - pads[2] - pads[3] + dils[1] * (kw - 1) + 1)
    out = []
    for d, o, s in zip(dflt, output_size, strides):
        if d < 1:
            raise ValueError("non-positive output extent %d" % d)
        if o and not d <= o < d + s:
            raise ValueError("output_size %d outside [%d, %d)" % (o, d, d + s))
        out.append(o or d)
    return tuple(out)


def _check(x, w, groups):
    x, w = np.asarray(x), np.asarray(w)
    assert x.ndim == 4 and w.ndim == 4 and x.shape[1] == w.shape[0] and x.shape[1] % groups == 0
    return x.astype(np.int64), w.astype(np.int64)


def _to_i32(acc):
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return acc.astype(np.int32)


def acc_scatter(x, w, pads, strides, dils, groups=1, output_size=(0, 0)):
    x, w = _check(x, w, groups)
    n, cin, h, wd = x.shape
    mg, kh, kw = w.shape[1:]
    cg = cin // groups
    oh, ow = out_dims(h, wd, kh, kw, pads, strides, dils, output_size)
    (sh, sw), (dh, dw), pt, pl = strides, dils, pads[0], pads[2]
    acc = np.zeros((n, groups * mg, oh, ow), np.int64)
    for g in range(groups):
        xg, wg = x[:, g * cg:(g + 1) * cg], w[g * cg:(g + 1) * cg]
        for r in range(kh):
            iy = np.arange(h)
            oy = iy * sh - pt + r * dh
            ky = (oy >= 0) & (oy < oh)
            for s in range(kw):
                ix = np.arange(wd)
                ox = ix * sw - pl + s * dw
                kx = (ox >= 0) & (ox < ow)
                if not ky.any() or not kx.any():
                    continue
                contrib = np.einsum("nchw,cm->nmhw", xg[:, :, iy[ky]][:, :, :, ix[kx]], wg[:, :, r, s])
                acc[:, g * mg:(g + 1) * mg, oy[ky][:, None], ox[kx][None, :]] += contrib
    return _to_i32(acc)


def acc_gather(x, w, pads, strides, dils, groups=1, output_size=(0, 0)):
    x, w = _check(x, w, groups)
    n, cin, h, wd = x.shape
    mg, kh, kw = w.shape[1:]
    cg = cin // groups
    oh, ow = out_dims(h, wd, kh, kw, pads, strides, dils, output_size)
    (sh, sw), (dh, dw), pt, pl = strides, dils, pads[0], pads[2]
    acc = np.zeros((n, groups * mg, oh, ow), np.int64)
    oy, ox = np.arange(oh), np.arange(ow)
    for r in range(kh):
        ty = oy + pt - r * dh
        ky = (ty >= 0) & (ty % sh == 0) & (ty // sh < h)
        for s in range(kw):
            tx = ox + pl - s * dw
            kx = (tx >= 0) & (tx % sw == 0) & (tx // sw < wd)
            if not ky.any() or not kx.any():
                continue
            iy, ix = ty[ky] // sh, tx[kx] // sw
            for g in range(groups):
                xg = x[:, g * cg:(g + 1) * cg][:, :, iy][:, :, :, ix]
                acc[:, g * mg:(g + 1) * mg, oy[ky][:, None], ox[kx][None, :]] += np.einsum(
                    "nchw,cm->nmhw", xg, w[g * cg:(g + 1) * cg, :, r, s])
    return _to_i32(acc)


def conv2d_transpose(plref, x, w, pads, strides, dils, groups, scale, bias, act, alpha, int8_out, output_size=(0, 0)):
    """The op with conv's epilogue: scale / bias are the FOLDED per-output-channel arrays (plref.fold_scales); bias None = zeros."""
    acc = acc_gather(x, w, pads, strides, dils, groups, output_size)
    b = np.zeros(acc.shape[1], np.float32) if bias is None else bias
    return plref.epilogue(acc, scale, b, act, alpha, int8_out)


# ------------------------------------------------------------------ networks with conv2d_transpose (workloads.unet_mini_net)
INT8_OPS = ("conv2d", "depthwise_conv2d", "fc", "conv2d_transpose")


def plan(net):
    """[(kind, dict)] in execution order, kind in {calib, op}: shuffle_oracle.plan's rules (the reference's kernel pick and cast
    placement) with conv2d_transpose among the int8 ops."""
    from shuffle_oracle import ins_of
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
        prec[o["name"]] = "i8" if int8_out else "f32"
    return steps


def forward(plref, net, image):
    """name -> tensor for every variable of the unfused lowered program ("<var>/precision_trans" for calib outputs): the frozen
    oracles' functions (plref's conv, pool and calib, shuffle_oracle.concat, interp_oracle.arg_max) and conv2d_transpose above,
    its scales folded by plref.fold_scales exactly as a conv's are."""
    from interp_oracle import arg_max
    from shuffle_oracle import concat
    T = {net["input"]: np.ascontiguousarray(image, np.float32)}
    out = {}

    def put(name, val):
        T[name] = out[name] = val

    for kind, s in plan(net):
        if kind == "calib":
            put(s["dst"], plref.calib_f32_to_i8(T[s["src"]], s["scale"]))
            continue
        o, ins = s["o"], s["ins"]
        t = o["op"]
        x = T[ins[0]]
        if t == "conv2d":
            cout, cg, k, _ = o["w"].shape
            p, d = o["pad"], o.get("dilation", 1)
            sh = plref.shape(x.shape[0], x.shape[1], x.shape[2], x.shape[3], cout, k, k, (p, p, p, p), (o["stride"],) * 2, (d, d), o["groups"])
            y, _ = plref.conv2d(sh, x, o["w"], o["bias"], float(o["in_scale"]), o["w_scale"], s["oscale"], o["act"], o["act_coef"], s["int8_out"])
            put(o["name"], y)
        elif t == "conv2d_transpose":
            p, d, g = o["pad"], o.get("dilation", 1), o["groups"]
            cout = o["w"].shape[1] * g
            sc, bi, alpha = plref.fold_scales(int(s["int8_out"]), float(o["in_scale"]), o["w_scale"], s["oscale"], o["bias"], cout, o["act"],
                                              o["act_coef"])
            put(o["name"], conv2d_transpose(plref, x, o["w"], (p, p, p, p), (o["stride"],) * 2, (d, d), g, sc, bi, o["act"], alpha,
                                            s["int8_out"], o["output_size"] or (0, 0)))
        elif t == "pool2d":
            p = o["pad"]
            put(o["name"], plref.pool2d(x, o["pooling_type"], (o["ksize"],) * 2, (o["stride"],) * 2, (p, p, p, p), exclusive=True, ceil_mode=False))
        elif t == "concat":
            put(o["name"], concat([T[v] for v in ins], o["axis"]))
        elif t == "arg_max":
            put(o["name"], arg_max(x, o["axis"], o["dtype"], o["keepdims"]))
        else:
            raise ValueError(t)
    return out
