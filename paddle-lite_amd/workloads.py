"""Synthetic INT8 workloads of BASELINE.json: the MobileNetV1 graph exactly as it reaches the kernel boundary after
the reference's passes (SURVEY.md Appendix B layer table + Appendix D program shape), with random-init weights.

  feed(fp32) -> io_copy h2d -> calib fp32->int8 -> conv2d 3x3s2 [int8_out, relu]
     -> 13 x { depthwise_conv2d 3x3 [int8_out, relu] -> conv2d 1x1 [int8_out, relu] }   (last 1x1: fp32_out)
     -> pool2d global avg (fp32) -> calib fp32->int8 -> fc [fp32out] -> softmax -> io_copy d2h

Layer shapes: lite/tests/benchmark/src/convolution_configs.h:355-379.  Scales follow the reference tests' convention
(in = 1/127 at the input, per-channel-varying weight scales as produced by conv_bn fusion — SURVEY.md A.9) and are
chosen so that every int8 activation tensor keeps a healthy spread (neither all-zero nor saturated).
"""
import numpy as np

# (cin, cout, stride) of the 13 depthwise-separable blocks
MBV1_BLOCKS = [(32, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2),
               (512, 512, 1), (512, 512, 1), (512, 512, 1), (512, 512, 1), (512, 512, 1), (512, 1024, 2), (1024, 1024, 1)]
NUM_CLASSES = 1000


def mobilenet_v1_layers(res=224):
    """[(name, op_type, cin, cout, k, stride, pad, groups, hin)] for the 27 convs."""
    layers = [("conv1", "conv2d", 3, 32, 3, 2, 1, 1, res)]
    h = (res + 2 - 3) // 2 + 1
    for i, (cin, cout, s) in enumerate(MBV1_BLOCKS):
        layers.append(("dw%d" % (i + 2), "depthwise_conv2d", cin, cin, 3, s, 1, cin, h))
        h = (h + 2 - 3) // s + 1
        layers.append(("pw%d" % (i + 2), "conv2d", cin, cout, 1, 1, 0, 1, h))
    return layers


def mobilenet_v1_macs(res=224):
    tot = {"pointwise": 0, "depthwise": 0, "first": 0}
    act_bytes = 0
    for (name, op, cin, cout, k, s, p, g, hin) in mobilenet_v1_layers(res):
        ho = (hin + 2 * p - k) // s + 1
        macs = ho * ho * cout * (cin // g) * k * k
        key = "first" if name == "conv1" else ("depthwise" if g > 1 else "pointwise")
        tot[key] += macs
        act_bytes += cin * hin * hin + cout * ho * ho
    tot["fc"] = 1024 * NUM_CLASSES
    tot["act_bytes"] = act_bytes
    return tot


def make_mobilenet_v1_weights(seed=1234, res=224):
    """Seeded random-init int8 weights, fp32 biases and scales for every layer."""
    rng = np.random.default_rng(seed)
    W = {}
    in_scale = np.float32(1.0 / 127)  # network input in [-1, 1]
    W["input_scale"] = in_scale
    sig_x = 73.0  # std of a uniform int8 input
    for (name, op, cin, cout, k, s, p, g, hin) in mobilenet_v1_layers(res):
        kk = (cin // g) * k * k
        w = rng.integers(-127, 128, (cout, cin // g, k, k)).astype(np.int8)
        # every activation tensor covers a real range of about +-4: out_scale = 4/127; the per-channel weight scales
        # (varying, as conv_bn fusion leaves them — SURVEY.md A.9) are sized so that the requantised int8 output has
        # a std of ~45 before relu: acc_std * in_scale * w_scale / out_scale = 45
        out_scale = np.float32(4.0 / 127)
        acc_std = np.sqrt(kk) * sig_x * 73.0
        var = (1.0 + (np.arange(cout) % 7) / 8.0) / 1.375
        w_scale = (var * 45.0 * float(out_scale) / (acc_std * float(in_scale))).astype(np.float32)
        bias = (rng.uniform(-0.5, 0.5, cout) * 45.0 * float(out_scale)).astype(np.float32)
        W[name] = dict(w=w, bias=bias, w_scale=w_scale, in_scale=in_scale, out_scale=out_scale)
        in_scale = out_scale
        sig_x = 30.0  # post-relu int8 activations: half-normal with the std above
    # fc: input = calib(pool(fp32 output of the last pointwise)); pooled relu outputs are positive, O(real_std)
    pool_scale = np.float32(W["pw14"]["out_scale"] * 60.0 / 127.0)
    W["pool_scale"] = pool_scale
    wf = rng.integers(-127, 128, (1024, NUM_CLASSES)).astype(np.int8)
    W["fc"] = dict(w=wf, bias=rng.uniform(-1, 1, NUM_CLASSES).astype(np.float32),
                   w_scale=((1.0 + (np.arange(NUM_CLASSES) % 5) / 8.0) / 127.0 / 32.0).astype(np.float32),
                   in_scale=pool_scale, out_scale=np.float32(1.0))
    return W


def build_mobilenet_v1(pred, W, batch, res=224):
    """Emit the Appendix-D program into a liteapi.Predictor.  Returns the output variable name."""
    from . import liteapi
    pred.add_feed("image", (batch, 3, res, res), liteapi.PREC_FLOAT)
    pred.add_io_copy("image", "image_dev", True)
    pred.add_calib("image_dev", "x0", float(W["input_scale"]), True)
    cur = "x0"
    layers = mobilenet_v1_layers(res)
    for i, (name, op, cin, cout, k, s, p, g, hin) in enumerate(layers):
        L = W[name]
        last = i == len(layers) - 1  # consumer pool2d is not enable_int8 -> fp32_out (static_kernel_pick_pass.cc:93-106)
        pred.add_conv(op, cur, name, L["w"], L["bias"], (s, s), (p, p, p, p), (1, 1), g, 1, 0.0, float(L["in_scale"]),
                      L["w_scale"], float(L["out_scale"]), not last)
        cur = name
    pred.add_global_avg_pool(cur, "pool")
    pred.add_calib("pool", "pool_i8", float(W["pool_scale"]), True)
    F = W["fc"]
    pred.add_fc("pool_i8", "logits", F["w"], F["bias"], float(F["in_scale"]), F["w_scale"], float(F["out_scale"]), False, False)
    pred.add_softmax("logits", "prob")
    pred.add_io_copy("prob", "prob_host", False)
    return "prob_host"


# =====================================================================================================================
# Generic op-list networks ("as the optimiser sees them after its fusion passes") for graph mode
# (lite/api/graph_builder.h): ResNet50 and MobileNetV2 of BASELINE.json configs C4 / C5, MobileNetV1 again in this form.
# Layer shapes: lite/tests/benchmark/src/convolution_configs.h:839-891 (ResNet50: stride 2 sits on the 3x3 conv of a
# stage's first block, shortcut = 1x1 stride-2 conv) and :381-466 (MobileNetV2, t/c/n/s table); PH/PW there are totals.
# An op is a dict:
#   conv2d / depthwise_conv2d: name=out, src, w [cout, cin/g, k, k] int8, bias, stride, pad, groups, act (0 none, 1 relu,
#                              2 relu6), act_coef, in_scale (the activation scale of its input tensor), w_scale [cout]
#   fc: src, w [k, n], bias, in_scale, w_scale [n]
#   pool2d: src, pooling_type, ksize, stride, pad, global_pooling
#   add: x, y, act ("" | "relu")      softmax: src
#   concat: srcs [..], axis      split: src, names [..] (name = names[0]), axis, num, sections      shuffle_channel: src, group
#   bilinear_interp / nearest_interp: src, out_h, out_w, align_corners, align_mode      arg_max: src, axis, dtype, keepdims
#   a conv with a dilation other than 1 carries `dilation` (both axes)
#   conv2d_transpose: conv2d's fields with w [cin, cout / g, k, k] (no flip), bias / w_scale per OUTPUT channel, and output_size
#                     (None, or (h, w))
# On the reference's ARM target pool2d and elementwise_add exist in fp32 only, so the kernel-pick
# rule gives the convs in front of them the fp32_out kernel and the consumers behind them a calib.
# =====================================================================================================================
class _NetGen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.ops = []
        self.act_scale = {}   # tensor -> quantisation scale its int8 consumers use (Input0_scale)
        self.sig_i8 = {}      # tensor -> rough std of its int8 image (sizes the synthetic weight scales)
        self.shape = {}       # tensor -> (c, h, w)

    def tensor(self, name, c, h, w, act_scale, sig_i8):
        self.shape[name] = (c, h, w)
        self.act_scale[name] = np.float32(act_scale)
        self.sig_i8[name] = sig_i8

    def conv(self, name, src, cout, k, stride, pad, groups=1, act=1, act_coef=0.0, out_range=4.0, op=None, headroom=1.0, bias_shift=0.0,
             dilation=1):
        cin, h, w = self.shape[src]
        kk = (cin // groups) * k * k
        wt = self.rng.integers(-127, 128, (cout, cin // groups, k, k)).astype(np.int8)
        in_scale = self.act_scale[src]
        out_scale = np.float32(out_range / 127.0)
        acc_std = np.sqrt(kk) * self.sig_i8[src] * 73.0
        var = (1.0 + (np.arange(cout) % 7) / 8.0) / 1.375
        # headroom > 1: the weight scales are sized for an int8 std of 45 / headroom (fewer saturated values)
        w_scale = (var * 45.0 / headroom * float(out_scale) / (acc_std * float(in_scale))).astype(np.float32)
        # bias_shift: the centre of the biases in units of the sizing rule's int8 spread (0: centred, as conv_bn fusion leaves a
        # batch norm without a learnt offset; > 0: a positive offset, so that fewer values of a relu tensor are zero)
        bias = ((self.rng.uniform(-0.5, 0.5, cout) + bias_shift) * 45.0 * float(out_scale)).astype(np.float32)
        if op is None:
            op = "depthwise_conv2d" if (groups == cin and groups == cout and groups > 1) else "conv2d"
        self.ops.append(dict(op=op, name=name, src=src, w=wt, bias=bias, stride=stride, pad=pad, groups=groups, act=act,
                             act_coef=float(act_coef), in_scale=in_scale, w_scale=w_scale))
        if dilation != 1:
            self.ops[-1]["dilation"] = int(dilation)
        ke = dilation * (k - 1) + 1
        ho = (h + 2 * pad - ke) // stride + 1
        wo = (w + 2 * pad - ke) // stride + 1
        self.tensor(name, cout, ho, wo, out_scale, (30.0 if act else 45.0) / headroom)
        return name

    def deconv(self, name, src, cout, k, stride, pad, groups=1, act=1, act_coef=0.0, out_range=4.0, headroom=1.0, bias_shift=0.0,
               output_size=None):
        """conv2d_transpose, sized as conv sizes a conv: an output sums cin / groups * ceil(k / stride)^2 products at most (the taps of
        its phase), fewer at the border and in the phases a k that stride does not divide leaves short."""
        cin, h, w = self.shape[src]
        taps = -(-k // stride)
        kk = (cin // groups) * taps * taps
        wt = self.rng.integers(-127, 128, (cin, cout // groups, k, k)).astype(np.int8)
        in_scale = self.act_scale[src]
        out_scale = np.float32(out_range / 127.0)
        acc_std = np.sqrt(kk) * self.sig_i8[src] * 73.0
        var = (1.0 + (np.arange(cout) % 7) / 8.0) / 1.375
        w_scale = (var * 45.0 / headroom * float(out_scale) / (acc_std * float(in_scale))).astype(np.float32)
        bias = ((self.rng.uniform(-0.5, 0.5, cout) + bias_shift) * 45.0 * float(out_scale)).astype(np.float32)
        self.ops.append(dict(op="conv2d_transpose", name=name, src=src, w=wt, bias=bias, stride=stride, pad=pad, groups=groups, act=act,
                             act_coef=float(act_coef), in_scale=in_scale, w_scale=w_scale,
                             output_size=None if output_size is None else tuple(int(v) for v in output_size)))
        ho, wo = ((h - 1) * stride - 2 * pad + k, (w - 1) * stride - 2 * pad + k) if output_size is None else output_size
        self.tensor(name, cout, int(ho), int(wo), out_scale, (30.0 if act else 45.0) / headroom)
        return name

    def pool(self, name, src, pooling_type, k, stride, pad, global_pooling=False, act_scale=None, sig_i8=40.0):
        c, h, w = self.shape[src]
        self.ops.append(dict(op="pool2d", name=name, src=src, pooling_type=pooling_type, ksize=k, stride=stride, pad=pad,
                             global_pooling=global_pooling))
        if global_pooling:
            self.tensor(name, c, 1, 1, np.float32(self.act_scale[src] * 100.0 / 127.0) if act_scale is None else act_scale, sig_i8)
        else:
            self.tensor(name, c, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1, self.act_scale[src],
                        self.sig_i8[src] * 1.3)
        return name

    def add(self, name, x, y, act=""):
        c, h, w = self.shape[x]
        self.ops.append(dict(op="add", name=name, x=x, y=y, act=act))
        # real-valued std of the sum = hypot of the operands' (int8 std x scale); quantise it so that the int8 image
        # has a std of ~45 before the relu, like every conv output
        real = float(np.hypot(self.sig_i8[x] * float(self.act_scale[x]), self.sig_i8[y] * float(self.act_scale[y])))
        self.tensor(name, c, h, w, np.float32(real / (28.0 if act else 45.0)), 42.0 if act else 45.0)
        return name

    def widen(self, name, f):
        """Quantise `name` over a range f times wider than the sizing rule gave it (fewer saturated values)."""
        self.act_scale[name] = np.float32(self.act_scale[name] * f)
        self.sig_i8[name] = self.sig_i8[name] / f
        return name

    def hard_swish(self, name, src, out_range=12.0):
        """fp32 op.  Its input is a conv output sized over [-8, 8] (std ~2.8: a real share of x <= -3, of the ramp and of x >= 3);
        its own int8 consumers quantise it over [-out_range, out_range], which holds the zero region and the linear region."""
        c, h, w = self.shape[src]
        self.ops.append(dict(op="hard_swish", name=name, src=src))
        self.tensor(name, c, h, w, np.float32(out_range / 127.0), 30.0)
        return name

    def hard_sigmoid(self, name, src):
        c, h, w = self.shape[src]
        self.ops.append(dict(op="hard_sigmoid", name=name, src=src))
        self.tensor(name, c, h, w, np.float32(1.0 / 127.0), 60.0)  # a gate in [0, 1]; only the fp32 multiply reads it
        return name

    def mul(self, name, x, y):
        """elementwise_mul, y [c, 1, 1] the gate of a squeeze-excite block (in [0, 1]): the product keeps x's range."""
        c, h, w = self.shape[x]
        assert self.shape[y] == (c, 1, 1), (self.shape[y], c)
        self.ops.append(dict(op="mul", name=name, x=x, y=y))
        self.tensor(name, c, h, w, self.act_scale[x], self.sig_i8[x] * 0.6)
        return name

    def concat(self, name, srcs, axis=1):
        """fp32 op along the channel axis.  Its int8 consumers quantise the whole tensor with ONE scale, which must hold every
        operand: the largest of the operands' scales (a smaller one would saturate the operand that was sized over the wider
        range); an operand of a smaller scale then fills that much less of the int8 range."""
        assert axis == 1 and len({self.shape[v][1:] for v in srcs}) == 1, [self.shape[v] for v in srcs]
        self.ops.append(dict(op="concat", name=name, srcs=list(srcs), axis=axis))
        scale = max(float(self.act_scale[v]) for v in srcs)
        cs = [self.shape[v][0] for v in srcs]
        ms = sum(c * (self.sig_i8[v] * float(self.act_scale[v]) / scale) ** 2 for c, v in zip(cs, srcs)) / sum(cs)
        _, h, w = self.shape[srcs[0]]
        self.tensor(name, sum(cs), h, w, np.float32(scale), float(np.sqrt(ms)))
        return name

    def split(self, names, src, axis=1, num=0, sections=()):
        """fp32 op: `num` equal parts of the channel axis, or `sections`; every part keeps the source's scale."""
        c, h, w = self.shape[src]
        assert axis == 1
        parts = [c // num] * num if num > 0 else list(sections)
        assert sum(parts) == c and len(parts) == len(names), (parts, c, names)
        self.ops.append(dict(op="split", name=names[0], names=list(names), src=src, axis=axis, num=num, sections=tuple(sections)))
        for n_, c_ in zip(names, parts):
            self.tensor(n_, c_, h, w, self.act_scale[src], self.sig_i8[src])
        return list(names)

    def shuffle(self, name, src, group):
        c, h, w = self.shape[src]
        assert c % group == 0, (c, group)
        self.ops.append(dict(op="shuffle_channel", name=name, src=src, group=group))
        self.tensor(name, c, h, w, self.act_scale[src], self.sig_i8[src])
        return name

    def interp(self, name, src, method, out_hw, align_corners=True, align_mode=1):
        """fp32 op, bilinear_interp | nearest_interp to out_hw (the reference's attribute defaults).  A resampled value lies between
        the source's values: the tensor keeps the source's scale and spread."""
        assert method in ("bilinear", "nearest")
        c, h, w = self.shape[src]
        oh, ow = (int(v) for v in out_hw)
        self.ops.append(dict(op=method + "_interp", name=name, src=src, out_h=oh, out_w=ow, align_corners=bool(align_corners),
                             align_mode=int(align_mode)))
        self.tensor(name, c, oh, ow, self.act_scale[src], self.sig_i8[src])
        return name

    def arg_max(self, name, src, axis=1, dtype=-1, keepdims=False):
        """The labels along the channel axis of [c, h, w]: int64 (dtype -1, 3) or int32 (2); no int8 op reads them."""
        assert axis == 1 and dtype in (-1, 2, 3)
        c, h, w = self.shape[src]
        self.ops.append(dict(op="arg_max", name=name, src=src, axis=axis, dtype=int(dtype), keepdims=bool(keepdims)))
        self.shape[name] = (1, h, w) if keepdims else (h, w)
        return name

    # ---- detection heads: fp32 ops on tensors that are no [c, h, w] feature maps.  self.shape holds their dims without the batch
    # axis; a tensor without one (prior boxes) is listed in self.batchless and keeps all its dims.  perm / shape / axis are the
    # op's attributes, over the full dims.
    def _full(self, v):
        return tuple(self.shape[v]) if v in getattr(self, "batchless", ()) else (1,) + tuple(self.shape[v])

    def _set_full(self, name, full, batchless):
        if batchless:
            self.batchless = getattr(self, "batchless", set()) | {name}
        self.shape[name] = tuple(full) if batchless else tuple(full[1:])
        return name

    def transpose(self, name, src, perm):
        full = self._full(src)
        assert sorted(perm) == list(range(len(full))) and (src in getattr(self, "batchless", ()) or perm[0] == 0), perm
        self.ops.append(dict(op="transpose", name=name, src=src, perm=tuple(int(p) for p in perm)))
        return self._set_full(name, [full[p] for p in perm], src in getattr(self, "batchless", ()))

    def reshape(self, name, src, shape):
        """The reference's shape attribute: 0 copies the input's dim at that place, one -1 is inferred."""
        full = self._full(src)
        batchless = src in getattr(self, "batchless", ())
        assert batchless or shape[0] == 0, shape
        out = [full[i] if d == 0 else d for i, d in enumerate(shape)]
        if -1 in out:
            out[out.index(-1)] = int(np.prod(full)) // int(np.prod([d for d in out if d != -1]))
        assert int(np.prod(out)) == int(np.prod(full)), (full, shape)
        self.ops.append(dict(op="reshape", name=name, src=src, shape=tuple(int(d) for d in shape)))
        return self._set_full(name, out, batchless)

    def join(self, name, srcs, axis):
        """concat of fp32 tensors nothing quantises (the joined heads, the prior boxes) along `axis` of their full dims."""
        fulls = [self._full(v) for v in srcs]
        batchless = srcs[0] in getattr(self, "batchless", ())
        out = list(fulls[0])
        out[axis] = sum(f[axis] for f in fulls)
        assert all(f[:axis] + f[axis + 1:] == fulls[0][:axis] + fulls[0][axis + 1:] for f in fulls), fulls
        self.ops.append(dict(op="concat", name=name, srcs=list(srcs), axis=int(axis)))
        return self._set_full(name, out, batchless)

    def prior_box(self, names, src, image, min_sizes, max_sizes, aspect_ratios, variances=(0.1, 0.1, 0.2, 0.2), flip=True, clip=False,
                  step_w=0.0, step_h=0.0, offset=0.5, min_max_aspect_ratios_order=False):
        """Boxes and Variances [H, W, A, 4] of the feature map src; A = (1 + the distinct ratios other than 1, twice with flip) per
        min_size + one per max_size."""
        _c, h, w = self.shape[src]
        ars = [1.0]
        for a in aspect_ratios:
            if not any(abs(a - b) < 1e-6 for b in ars):
                ars += [a, 1.0 / a] if flip else [a]
        num = len(ars) * len(min_sizes) + len(max_sizes)
        self.ops.append(dict(op="prior_box", name=names[0], names=list(names), src=src, image=image, min_sizes=tuple(min_sizes),
                             max_sizes=tuple(max_sizes), aspect_ratios=tuple(aspect_ratios), variances=tuple(variances), flip=bool(flip),
                             clip=bool(clip), step_w=float(step_w), step_h=float(step_h), offset=float(offset),
                             min_max_aspect_ratios_order=bool(min_max_aspect_ratios_order)))
        for n_ in names:
            self._set_full(n_, (h, w, num, 4), True)
        return list(names)

    def box_coder(self, name, prior, target, prior_var="", variance=None, axis=0, normalized=True):
        """decode_center_size of target [P, 4] per image against prior [P, 4]."""
        self.ops.append(dict(op="box_coder", name=name, prior=prior, prior_var=prior_var, target=target,
                             variance=None if variance is None else tuple(variance), axis=int(axis), normalized=bool(normalized)))
        self.shape[name] = self.shape[target]
        return name

    def yolo_box(self, names, src, img_size, anchors, class_num, conf_thresh, downsample_ratio, clip_bbox=True, scale_x_y=1.0):
        """names (Boxes [P, 4], Scores [P, class_num]) per image of the head map src [an * (5 + class_num), h, w], P = an * h * w; img_size:
        the int32 [N, 2] feed."""
        c, h, w = self.shape[src]
        an = len(anchors) // 2
        assert len(anchors) % 2 == 0 and c == an * (5 + class_num), (c, anchors, class_num)
        self.ops.append(dict(op="yolo_box", name=names[0], names=list(names), src=src, img_size=img_size, anchors=tuple(int(a) for a in anchors),
                             class_num=int(class_num), conf_thresh=float(conf_thresh), downsample_ratio=int(downsample_ratio),
                             clip_bbox=bool(clip_bbox), scale_x_y=float(scale_x_y)))
        self.shape[names[0]] = (an * h * w, 4)
        self.shape[names[1]] = (an * h * w, int(class_num))
        return list(names)

    def multiclass_nms(self, name, boxes, scores, background_label, score_threshold, nms_top_k, nms_threshold, keep_top_k, normalized=True,
                       nms_eta=1.0, index=""):
        """name [keep_top_k, 6] per image padded with -1, name + "/count" the per-image counts."""
        self.ops.append(dict(op="multiclass_nms", name=name, boxes=boxes, scores=scores, background_label=int(background_label),
                             score_threshold=float(score_threshold), nms_top_k=int(nms_top_k), nms_threshold=float(nms_threshold),
                             nms_eta=float(nms_eta), keep_top_k=int(keep_top_k), normalized=bool(normalized), index=index))
        self.shape[name] = (int(keep_top_k), 6)
        self.shape[name + "/count"] = ()
        return name

    def fc(self, name, src, n):
        c, h, w = self.shape[src]
        k = c * h * w
        wf = self.rng.integers(-127, 128, (k, n)).astype(np.int8)
        self.ops.append(dict(op="fc", name=name, src=src, w=wf, bias=self.rng.uniform(-1, 1, n).astype(np.float32),
                             in_scale=self.act_scale[src],
                             w_scale=((1.0 + (np.arange(n) % 5) / 8.0) / 127.0 / 32.0).astype(np.float32)))
        self.tensor(name, n, 1, 1, np.float32(1.0), 30.0)
        return name

    def softmax(self, name, src):
        self.ops.append(dict(op="softmax", name=name, src=src))
        self.shape[name] = self.shape[src]
        return name


def _finish(g, res, out):
    return dict(ops=g.ops, input="image", input_shape=(3, res, res), output=out, shapes=dict(g.shape))


def resnet50_net(seed=50, res=224, num_classes=NUM_CLASSES):
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    x = g.conv("conv1", "image", 64, 7, 2, 3, act=1)
    x = g.pool("pool1", x, "max", 3, 2, 1)
    for si, (width, blocks, stride) in enumerate([(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)]):
        for b in range(blocks):
            p = "res%d%s" % (si + 2, "abcdef"[b])
            s = stride if b == 0 else 1
            y = g.conv(p + "_branch2a", x, width, 1, 1, 0, act=1)
            y = g.conv(p + "_branch2b", y, width, 3, s, 1, act=1)
            y = g.conv(p + "_branch2c", y, 4 * width, 1, 1, 0, act=0)
            sc = g.conv(p + "_branch1", x, 4 * width, 1, s, 0, act=0) if b == 0 else x
            x = g.add(p, sc, y, act="relu")
    x = g.pool("pool5", x, "avg", 7, 1, 0, global_pooling=True)
    x = g.fc("fc", x, num_classes)
    x = g.softmax("prob", x)
    return _finish(g, res, x)


def resnext50_net(seed=54, res=224, groups=32, base_width=4, num_classes=NUM_CLASSES):
    """ResNeXt50 (32x4d by default): resnet50_net with branch2a / branch2b of groups * base_width * 2^stage channels (128, 256,
    512, 1024) and `groups` on the 3x3 branch2b; the stride sits on the 3x3, as there."""
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    x = g.conv("conv1", "image", 64, 7, 2, 3, act=1)
    x = g.pool("pool1", x, "max", 3, 2, 1)
    for si, (width, blocks, stride) in enumerate([(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)]):
        inner = groups * base_width * 2 ** si
        for b in range(blocks):
            p = "res%d%s" % (si + 2, "abcdef"[b])
            s = stride if b == 0 else 1
            y = g.conv(p + "_branch2a", x, inner, 1, 1, 0, act=1)
            y = g.conv(p + "_branch2b", y, inner, 3, s, 1, groups=groups, act=1)
            y = g.conv(p + "_branch2c", y, 4 * width, 1, 1, 0, act=0)
            sc = g.conv(p + "_branch1", x, 4 * width, 1, s, 0, act=0) if b == 0 else x
            x = g.add(p, sc, y, act="relu")
    x = g.pool("pool5", x, "avg", 7, 1, 0, global_pooling=True)
    x = g.fc("fc", x, num_classes)
    x = g.softmax("prob", x)
    return _finish(g, res, x)


MBV2_SETTING = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]


def mobilenet_v2_net(seed=52, res=224, num_classes=NUM_CLASSES):
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    R6 = dict(act=2, act_coef=6.0, out_range=8.0)  # relu6 tensors quantised over [-8, 8]: the clip at 6 is visible in int8
    x = g.conv("conv1", "image", 32, 3, 2, 1, **R6)
    cin, bi = 32, 0
    for (t, c, n, s) in MBV2_SETTING:
        for i in range(n):
            bi += 1
            p = "b%d" % bi
            stride = s if i == 0 else 1
            y = x
            if t != 1:
                y = g.conv(p + "_expand", y, cin * t, 1, 1, 0, **R6)
            y = g.conv(p + "_dw", y, cin * t, 3, stride, 1, groups=cin * t, **R6)
            y = g.conv(p + "_project", y, c, 1, 1, 0, act=0)
            x = g.add(p + "_add", x, y) if (stride == 1 and cin == c) else y
            cin = c
    x = g.conv("conv_last", x, 1280, 1, 1, 0, **R6)
    x = g.pool("pool", x, "avg", g.shape[x][1], 1, 0, global_pooling=True)
    x = g.fc("fc", x, num_classes)
    x = g.softmax("prob", x)
    return _finish(g, res, x)


# MobileNetV3 (lite/tests/benchmark/src/convolution_configs.h:467-653 lists every conv, the excite convs on 1 x 1 planes included;
# block structure as published, Howard et al. 2019, tables 1 and 2): (kernel, expanded, out, squeeze-excite, hard_swish, stride)
MBV3_LARGE = [(3, 16, 16, 0, 0, 1), (3, 64, 24, 0, 0, 2), (3, 72, 24, 0, 0, 1), (5, 72, 40, 1, 0, 2), (5, 120, 40, 1, 0, 1),
              (5, 120, 40, 1, 0, 1), (3, 240, 80, 0, 1, 2), (3, 200, 80, 0, 1, 1), (3, 184, 80, 0, 1, 1), (3, 184, 80, 0, 1, 1),
              (3, 480, 112, 1, 1, 1), (3, 672, 112, 1, 1, 1), (5, 672, 160, 1, 1, 2), (5, 960, 160, 1, 1, 1), (5, 960, 160, 1, 1, 1)]
MBV3_SMALL = [(3, 16, 16, 1, 0, 2), (3, 72, 24, 0, 0, 2), (3, 88, 24, 0, 0, 1), (5, 96, 40, 1, 1, 2), (5, 240, 40, 1, 1, 1),
              (5, 240, 40, 1, 1, 1), (5, 120, 48, 1, 1, 1), (5, 144, 48, 1, 1, 1), (5, 288, 96, 1, 1, 2), (5, 576, 96, 1, 1, 1),
              (5, 576, 96, 1, 1, 1)]
MBV3_HEAD = {"large": (960, 1280), "small": (576, 1024)}


def mbv3_squeeze_channels(c):
    """make_divisible(c / 4, 8): 16 -> 8, 72 -> 24, 96 -> 24, 120 -> 32, 144 -> 40, 240 -> 64, 288 -> 72, 480 -> 120 ..."""
    v = max(8, int(c / 4 + 4) // 8 * 8)
    return v + 8 if v < 0.9 * c / 4 else v


def mobilenet_v3_net(variant="large", seed=53, res=224, num_classes=NUM_CLASSES):
    """MobileNetV3-Large / -Small as the reference's optimiser leaves it: relu is fused into the int8 convs, hard_swish and
    hard_sigmoid are fp32 ops of their own (conv_activation_fuse_pass.cc:26-44), the squeeze-excite gate is applied by an fp32
    elementwise_mul.  The convs in front of hard_swish are sized over [-8, 8] (both clamps of the op see data), the second
    excite conv too (the gate 0.2 x + 0.5 reaches 0 and 1 at -+2.5)."""
    table = {"large": MBV3_LARGE, "small": MBV3_SMALL}[variant]
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    HS = dict(act=0, out_range=8.0)
    x = g.hard_swish("conv1_hs", g.conv("conv1", "image", 16, 3, 2, 1, **HS))
    cin = 16
    for bi, (k, exp, cout, se, hs, stride) in enumerate(table):
        p = "b%d" % (bi + 1)
        act = HS if hs else dict(act=1, headroom=1.6)
        y = x
        if exp != cin:
            y = g.conv(p + "_expand", y, exp, 1, 1, 0, **act)
            if hs:
                y = g.hard_swish(p + "_expand_hs", y)
        # (the depthwise taps see the hard_swish output, whose int8 rms the rule overestimates: sized over [-16, 16])
        y = g.conv(p + "_dw", y, exp, k, stride, k // 2, groups=exp, **(dict(act=0, out_range=16.0) if hs else act))
        if hs:
            y = g.hard_swish(p + "_dw_hs", y)
        if se:
            # a plane's mean lies inside the plane's own range: the pooled tensor keeps its source's scale
            q = g.pool(p + "_se_pool", y, "avg", g.shape[y][1], 1, 0, global_pooling=True, act_scale=g.act_scale[y] * 1.5, sig_i8=14.0)
            q = g.conv(p + "_se_reduce", q, mbv3_squeeze_channels(exp), 1, 1, 0, act=1, headroom=2.0)
            q = g.conv(p + "_se_expand", q, exp, 1, 1, 0, **HS)
            q = g.hard_sigmoid(p + "_se_gate", q)
            y = g.mul(p + "_se_mul", y, q)
        y = g.conv(p + "_project", y, cout, 1, 1, 0, act=0, headroom=1.6)
        x = g.widen(g.add(p + "_add", x, y), 1.5) if (stride == 1 and cin == cout) else y
        cin = cout
    c_last, c_head = MBV3_HEAD[variant]
    x = g.hard_swish("conv_last_hs", g.conv("conv_last", x, c_last, 1, 1, 0, **HS))
    x = g.pool("pool", x, "avg", g.shape[x][1], 1, 0, global_pooling=True, act_scale=g.act_scale[x], sig_i8=20.0)
    x = g.hard_swish("conv_head_hs", g.conv("conv_head", x, c_head, 1, 1, 0, **HS))
    x = g.fc("fc", x, num_classes)
    x = g.softmax("prob", x)
    return _finish(g, res, x)


# ShuffleNetV2 (Ma et al. 2018, table 5; the reference runs it as lite/api/shufflenetv2_test.cc): stage widths by scale
SHUFFLENET_V2_WIDTHS = {0.5: (48, 96, 192), 1.0: (116, 232, 464), 1.5: (176, 352, 704), 2.0: (244, 488, 976)}
SHUFFLENET_V2_REPEATS = (4, 8, 4)


def shufflenet_v2_net(scale=1.0, seed=55, res=224, num_classes=NUM_CLASSES):
    """ShuffleNetV2 as the reference's optimiser leaves it: relu fused into the int8 convs, shuffle_channel already fused from
    reshape / transpose / reshape (shuffle_channel_fuse_pass.cc), concat / shuffle_channel / split fp32 ops.  A stride-1 unit
    splits its input in two, runs conv1x1+relu -> dw3x3 -> conv1x1+relu on the second half, concatenates and shuffles (group 2); a
    stride-2 unit runs dw3x3 s2 -> conv1x1+relu on the left, conv1x1+relu -> dw3x3 s2 -> conv1x1+relu on the right.  Every conv
    output is sized over [-4, 4], so the two operands of every concat share one scale."""
    widths = SHUFFLENET_V2_WIDTHS[scale]
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    x = g.conv("conv1", "image", 24, 3, 2, 1, act=1)
    x = g.pool("pool1", x, "max", 3, 2, 1)
    cin = 24
    # Sizing (checked on the oracle, tests/test_shufflenet_host.py, against MobileNetV2's worst tensor).  A depthwise conv
    # without an activation saturates on both sides, and its taps see relu outputs of neighbouring pixels, whose sum spreads
    # about 1.6 times wider than the rule for independent taps says: its weight scales are sized for a third of the usual int8
    # spread and the spread its reader is sized by is corrected.  The 1x1 convs in front of a concat keep a quarter of headroom,
    # so that the concat's one scale holds both operands.  The first 1x1 conv of a branch has as few as 24 channels, and a relu
    # channel's share of zeros is decided by the sign of its offset: with biases centred on zero a narrow tensor can be mostly
    # zeros by the luck of its weights, whatever the scales.  Its biases are centred a quarter of the spread above zero (a batch
    # norm with a positive learnt offset), with the headroom that offset needs.
    DW = dict(act=0, headroom=3.0)
    PW = dict(act=1, headroom=1.25)
    PW1 = dict(act=1, headroom=1.6, bias_shift=0.25)

    def dw(name):
        g.sig_i8[name] *= 1.6
        return name
    for si, (width, reps) in enumerate(zip(widths, SHUFFLENET_V2_REPEATS)):
        h = width // 2
        for u in range(reps):
            p = "s%du%d" % (si + 2, u + 1)
            if u == 0:  # stride 2: both branches read the whole input
                left = dw(g.conv(p + "_l_dw", x, cin, 3, 2, 1, groups=cin, **DW))
                left = g.conv(p + "_l_pw", left, h, 1, 1, 0, **PW)
                y = g.conv(p + "_r_pw1", x, h, 1, 1, 0, **PW1)
                y = dw(g.conv(p + "_r_dw", y, h, 3, 2, 1, groups=h, **DW))
            else:
                left, right = g.split([p + "_x1", p + "_x2"], x, 1, num=2)
                y = g.conv(p + "_r_pw1", right, h, 1, 1, 0, **PW1)
                y = dw(g.conv(p + "_r_dw", y, h, 3, 1, 1, groups=h, **DW))
            y = g.conv(p + "_r_pw2", y, h, 1, 1, 0, **PW)
            x = g.shuffle(p + "_shuffle", g.concat(p + "_concat", [left, y], 1), 2)
            cin = width
    x = g.conv("conv5", x, 2048 if scale == 2.0 else 1024, 1, 1, 0, act=1)
    x = g.pool("pool", x, "avg", g.shape[x][1], 1, 0, global_pooling=True)
    x = g.fc("fc", x, num_classes)
    x = g.softmax("prob", x)
    return _finish(g, res, x)


# SqueezeNet v1.1 (Iandola et al. 2016, the v1.1 revision: pools behind conv1, fire3 and fire5): (squeeze, expand) widths of fire2..9
SQUEEZENET_V1_1_FIRES = [(16, 64), (16, 64), (32, 128), (32, 128), (48, 192), (48, 192), (64, 256), (64, 256)]


def _spread(g, name, f):
    """The int8 spread the readers of `name` are sized by is f times what the rule for independent taps gave it."""
    g.sig_i8[name] *= f
    return name


def squeezenet_v1_1_net(seed=56, res=224, num_classes=NUM_CLASSES):
    """SqueezeNet v1.1 as the reference's optimiser leaves it: relu fused into the int8 convs, concat and pool2d fp32 ops.  A fire
    module is a squeeze 1x1 conv, then an expand 1x1 and an expand 3x3 (pad 1) conv on it, and the concat of the two.  A max pool
    and a concat of relu tensors spread wider than the sizing rule for independent taps says (checked on the oracle,
    tests/test_squeezenet_host.py, against MobileNetV2's worst tensor): the spread a reader is sized by is corrected, 1.6 times for
    a max pool output, 1.4 times for a concat output and for a squeeze conv output, as shufflenet_v2_net does for its depthwise
    outputs.  The global average pool's output is [N, classes, 1, 1] and softmax runs along the last axis, as everywhere in this
    project: the tensor that carries the network's result is pool10."""
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    x = g.conv("conv1", "image", 64, 3, 2, 1, act=1)
    x = _spread(g, g.pool("pool1", x, "max", 3, 2, 0), 1.6)
    for i, (sq, ex) in enumerate(SQUEEZENET_V1_1_FIRES):
        p = "fire%d" % (i + 2)
        s = _spread(g, g.conv(p + "_squeeze", x, sq, 1, 1, 0, act=1), 1.4)
        a = g.conv(p + "_expand1x1", s, ex, 1, 1, 0, act=1)
        b = g.conv(p + "_expand3x3", s, ex, 3, 1, 1, act=1)
        x = _spread(g, g.concat(p + "_concat", [a, b], 1), 1.4)
        if p in ("fire3", "fire5"):
            x = _spread(g, g.pool("pool%d" % (i + 2), x, "max", 3, 2, 0), 1.6)
    x = g.conv("conv10", x, num_classes, 1, 1, 0, act=1)
    x = g.pool("pool10", x, "avg", g.shape[x][1], 1, 0, global_pooling=True)
    x = g.softmax("prob", x)
    return _finish(g, res, x)


# (1x1, 3x3 reduce, 3x3, 5x5 reduce, 5x5, pool projection) channels of the two blocks of inception_mini_net
INCEPTION_MINI_BLOCKS = [(16, 24, 32, 4, 8, 8), (32, 32, 48, 8, 24, 16)]


def inception_mini_net(seed=57, res=64, num_classes=10):
    """Two GoogLeNet-style blocks (Szegedy et al. 2014) behind a two-conv stem: branches 1x1 | 1x1 -> 3x3 | 1x1 -> 5x5 | max pool
    3x3 s1 -> 1x1, every conv with relu, and the concat of the four.  The smallest network with a four-operand concat, and with a
    max pool that reads a concat beside int8 convs that read it through one calib.  Sizing: the spread corrections of
    squeezenet_v1_1_net; the narrow 5x5 reduce conv as shufflenet_v2_net's first 1x1 conv of a branch; a 3x3 stride-1 max pool
    spreads one saturated value over nine windows, so a block's input is quantised over a range 1.5 times wider."""
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    x = g.conv("conv1", "image", 32, 3, 2, 1, act=1)
    x = g.conv("conv2", x, 64, 3, 1, 1, act=1)
    for bi, (c1, r3, c3, r5, c5, cp) in enumerate(INCEPTION_MINI_BLOCKS):
        p = "inc%d" % (bi + 1)
        g.widen(x, 1.5)
        b1 = g.conv(p + "_1x1", x, c1, 1, 1, 0, act=1)
        b3 = g.conv(p + "_3x3", g.conv(p + "_3x3_reduce", x, r3, 1, 1, 0, act=1), c3, 3, 1, 1, act=1)
        b5 = g.conv(p + "_5x5", g.conv(p + "_5x5_reduce", x, r5, 1, 1, 0, act=1, headroom=1.6, bias_shift=0.25), c5, 5, 1, 2, act=1)
        bp = g.conv(p + "_pool_proj", _spread(g, g.pool(p + "_pool", x, "max", 3, 1, 1), 1.6), cp, 1, 1, 0, act=1)
        x = _spread(g, g.concat(p + "_concat", [b1, b3, b5, bp], 1), 1.4)
    x = g.pool("pool", x, "avg", g.shape[x][1], 1, 0, global_pooling=True)
    x = g.fc("fc", x, num_classes)
    x = g.softmax("prob", x)
    return _finish(g, res, x)


def seg_mini_net(seed=58, res=64, num_classes=19):
    """A DeepLabV3+-shaped segmentation net (Chen et al. 2018) small enough for the CPU oracle: a depthwise-separable encoder to
    res / 8, an ASPP of a 1x1 and two dilated 3x3 convs with their 1x1 projection, a decoder that raises the resolution twice
    (bilinear to the `low` features at res / 4 and concat with their 1x1 reduction, then nearest to res / 2) and a head that
    resamples the class logits to the input size and takes the per-pixel arg_max.  The first network here with interp ops, dilated
    convs and an integer result.  Lowering with every fusion on: L takes both concats, N the nearest interp (a conv reads it), M the
    head; the first bilinear interp feeds a concat and stays as it is.
    Sizing: the spread corrections of squeezenet_v1_1_net for the concats (1.4), a depthwise conv sized with half as much
    headroom again (its 9 taps see relu outputs of neighbouring pixels, whose sum spreads wider than the rule for independent taps
    says, as shufflenet_v2_net's do), and an ASPP input quantised over a range 1.5
    times wider, as inception_mini_net widens a block's input that several branches read.  The logits are fp32 and keep their sign
    (no activation): tests/test_interp_host.py states the worst saturated and zero shares of the int8 tensors."""
    assert res % 8 == 0
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    x = g.conv("stem", "image", 16, 3, 2, 1, act=1)

    def block(p, x, cout, stride):
        c = g.shape[x][0]
        d = _spread(g, g.conv(p + "_dw", x, c, 3, stride, 1, groups=c, act=1, headroom=1.5), 1.4 * 1.5)
        return g.conv(p + "_pw", d, cout, 1, 1, 0, act=1)

    low = block("enc1", x, 24, 2)                      # res / 4
    x = block("enc3", block("enc2", low, 64, 2), 64, 1)  # res / 8
    g.widen(x, 1.5)
    a1 = g.conv("aspp_1x1", x, 32, 1, 1, 0, act=1)
    a2 = g.conv("aspp_d2", x, 32, 3, 1, 2, act=1, dilation=2)
    a3 = g.conv("aspp_d3", x, 32, 3, 1, 3, act=1, dilation=3)
    x = _spread(g, g.concat("aspp_concat", [a1, a2, a3], 1), 1.4)
    x = g.conv("aspp_project", x, 32, 1, 1, 0, act=1)
    x = g.interp("dec_up1", x, "bilinear", g.shape[low][1:], align_corners=False, align_mode=1)
    r = g.conv("dec_low", low, 16, 1, 1, 0, act=1)
    x = _spread(g, g.concat("dec_concat", [x, r], 1), 1.4)
    x = g.conv("dec_conv1", x, 32, 3, 1, 1, act=1)
    x = g.interp("dec_up2", x, "nearest", (res // 2, res // 2), align_corners=False)
    x = g.conv("dec_conv2", x, 32, 3, 1, 1, act=1)
    x = g.conv("logits", x, num_classes, 1, 1, 0, act=0)
    x = g.interp("logits_up", x, "bilinear", (res, res), align_corners=True)
    x = g.arg_max("label", x, 1, dtype=-1)
    return _finish(g, res, x)


def unet_mini_net(seed=60, res=64, num_classes=4):
    """A U-Net (Ronneberger et al. 2015) small enough for the CPU oracle: two encoder stages of 3x3 convs and a 2x2 max pool, a
    bottleneck at res / 4, two decoder stages conv2d_transpose -> concat with the encoder's skip tensor -> 3x3 conv, a 1x1 classifier
    and the per-pixel arg_max.  The first network here with a learned upsampling: dec2_up is k 2 s 2 p 0 (128 -> 64 channels, every
    output one tap), dec1_up is k 4 s 2 p 1 (64 -> 32, four taps), so both phase patterns of the MFMA route are in one program.
    Both read an int8 tensor and write fp32 (a concat reads them).  Lowering with every fusion on: L takes both concats (concat/int8)
    and the two max pools behind fp32 convs stay fp32 readers of tensors a concat reads too.
    Sizing: the spread corrections of squeezenet_v1_1_net for the concats (1.4); the second max pool keeps the largest of four
    relu outputs of a 64-channel conv, so its readers quantise it over a range 1.4 times wider (as inception_mini_net widens a
    tensor behind a max pool), and the bottleneck conv that reads it and dec2_up behind that are sized with 1.3 and 1.25 times the headroom.  tests/test_deconv_host.py states the worst saturated and zero shares of the int8 tensors."""
    assert res % 4 == 0
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    x = g.conv("enc1_conv1", "image", 32, 3, 1, 1, act=1)
    skip1 = g.conv("enc1_conv2", x, 32, 3, 1, 1, act=1)
    x = g.pool("enc1_pool", skip1, "max", 2, 2, 0)
    skip2 = g.conv("enc2_conv", x, 64, 3, 1, 1, act=1)
    x = g.widen(g.pool("enc2_pool", skip2, "max", 2, 2, 0), 1.4)
    x = g.conv("bottleneck", x, 128, 3, 1, 1, act=1, headroom=1.3)
    x = g.deconv("dec2_up", x, 64, 2, 2, 0, act=1, headroom=1.25)
    x = _spread(g, g.concat("dec2_concat", [x, skip2], 1), 1.4)
    x = g.conv("dec2_conv", x, 64, 3, 1, 1, act=1)
    x = g.deconv("dec1_up", x, 32, 4, 2, 1, act=1)
    x = _spread(g, g.concat("dec1_concat", [x, skip1], 1), 1.4)
    x = g.conv("dec1_conv", x, 32, 3, 1, 1, act=1)
    x = g.conv("logits", x, num_classes, 1, 1, 0, act=0)
    x = g.arg_max("label", x, 1, dtype=-1)
    return _finish(g, res, x)


def ssd_mini_net(seed=59, res=96, num_classes=21, conf_range=12.0):
    """An SSD-shaped detector (Liu et al. 2016) on a MobileNetV1-style backbone, small enough for the CPU oracle: depthwise-separable
    blocks to res / 8 (12 x 12 at res 96), / 16, / 32 and a 3x3 conv without padding behind them (1 x 1 at res 96); on each of the
    four maps a 3x3 pad-1 `loc` conv (A * 4 channels) and `conf` conv (A * num_classes), both linear with fp32 output, and a
    prior_box with SSD's schedule (sizes from 0.2 to 0.9 of the image, ratios {2} on the first and last map, {2, 3} between:
    A = 4 / 6).  The heads are joined as the reference's SSD models join them: transpose(0,2,3,1) -> reshape([0,-1,4 | classes]) ->
    concat(axis 1); the prior boxes and variances reshape([-1,4]) -> concat(axis 0).  box_coder decodes with the prior variances,
    softmax runs over the classes, transpose(0,2,1) brings the probabilities to [N, C, P] and multiclass_nms (background 0, score
    threshold 0.01, top 400, IoU 0.45, keep 200, normalized) writes "det" and "det/count".  The first network here whose result
    is a list of boxes.  Every feature map has a prior_box (an fp32 op) among its readers, so the kernel pick gives its conv the
    fp32_out kernel and the convs that read it a calib, as for pool2d.  conf_range: the range the class logits are sized over (the
    wider, the fewer probabilities pass the score threshold).  Random weights give every class some prior with a probability above
    0.01, so the biases of the LAST class are lowered by 1.5 conf_range on every map: a class the net never predicts, as a trained
    detector has for most images.  tests/test_detection_host.py states what the NMS of the committed seed then sees."""
    assert res >= 65, "the last map needs 3 x 3 pixels"
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    x = g.conv("stem", "image", 16, 3, 2, 1, act=1)

    def block(p, x, cout, stride):
        c = g.shape[x][0]
        d = _spread(g, g.conv(p + "_dw", x, c, 3, stride, 1, groups=c, act=1, headroom=1.5), 1.4 * 1.5)
        return g.conv(p + "_pw", d, cout, 1, 1, 0, act=1)

    x = block("b2", block("b1", x, 32, 2), 64, 2)      # res / 8
    maps = [x]
    maps.append(block("b3", maps[-1], 128, 2))          # res / 16
    maps.append(block("b4", maps[-1], 128, 2))          # res / 32
    maps.append(g.conv("extra", maps[-1], 64, 3, 1, 0, act=1))
    m = len(maps)
    sizes = [res * (0.2 + 0.7 * k / (m - 1)) for k in range(m)] + [float(res)]
    locs, confs, pboxes, pvars = [], [], [], []
    for k, f in enumerate(maps):
        ratios = (2.0,) if k in (0, m - 1) else (2.0, 3.0)
        a = 2 + 2 * len(ratios)
        tag = "f%d" % k
        loc = g.conv(tag + "_loc", f, a * 4, 3, 1, 1, act=0, out_range=2.0)
        conf = g.conv(tag + "_conf", f, a * num_classes, 3, 1, 1, act=0, out_range=conf_range)
        g.ops[-1]["bias"][num_classes - 1::num_classes] -= np.float32(1.5 * conf_range)  # channel a * num_classes + class
        locs.append(g.reshape(tag + "_loc_flat", g.transpose(tag + "_loc_nhwc", loc, (0, 2, 3, 1)), (0, -1, 4)))
        confs.append(g.reshape(tag + "_conf_flat", g.transpose(tag + "_conf_nhwc", conf, (0, 2, 3, 1)), (0, -1, num_classes)))
        b, v = g.prior_box([tag + "_prior", tag + "_prior_var"], f, "image", (sizes[k],), (sizes[k + 1],), ratios)
        pboxes.append(g.reshape(tag + "_prior_flat", b, (-1, 4)))
        pvars.append(g.reshape(tag + "_prior_var_flat", v, (-1, 4)))
    loc = g.join("loc", locs, 1)
    conf = g.join("conf", confs, 1)
    priors = g.join("priors", pboxes, 0)
    prior_vars = g.join("prior_vars", pvars, 0)
    boxes = g.box_coder("boxes", priors, loc, prior_var=prior_vars, axis=0, normalized=True)
    prob = g.softmax("prob", conf)
    scores = g.transpose("scores", prob, (0, 2, 1))
    det = g.multiclass_nms("det", boxes, scores, 0, 0.01, 400, 0.45, 200, normalized=True)
    return _finish(g, res, det)


COCO_ANCHORS = (10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326)  # YOLOv3 at 416 (Redmon & Farhadi 2018)


def yolov3_mini_net(seed=61, res=96, num_classes=20, obj_shift=1.4, head_range=6.0):
    """A YOLOv3-shaped detector (Redmon & Farhadi 2018) small enough for the CPU oracle.  Backbone, darknet-style: a 3x3 stem, then
    five 3x3 stride-2 downsampling convs, each followed by a residual block 1x1 (half the channels) -> 3x3 with an elementwise_add
    that has no activation; LeakyReLU 0.1 on every conv.  The maps of stride 8 / 16 / 32 (12 x 12, 6 x 6, 3 x 3 at res 96) feed the
    neck: 1x1 conv -> nearest_interp x2 -> concat with the finer map -> 3x3 conv, twice.  Three linear 1x1 head convs with fp32
    output write 3 * (5 + num_classes) channels; yolo_box decodes each map with its three of the nine COCO anchors scaled from 416 to
    res, downsample_ratio 32 / 16 / 8, conf_thresh 0.01 and clip_bbox; the Boxes and the Scores are concatenated along axis 1
    (coarsest map first, as the reference's YOLOv3 models list them), the scores go through transpose(0,2,1), and multiclass_nms
    (no background class, score threshold 0.01, top 400, IoU 0.45, keep 100, not normalized) writes "det" and "det/count".
    P = 3 * (9 + 36 + 144) = 567 at res 96.  The second input is "img_size", int32 [N, 2] (net["img_size"]).
    The head logits are sized over [-head_range, head_range]; random weights would put half of all cells above any threshold, so the
    objectness biases are lowered by obj_shift * head_range: a clear share of cells on each side of conf_thresh, as a trained
    detector leaves most cells empty.  tests/test_yolo_plugin_host.py states what the NMS of the committed seed then sees."""
    assert res % 32 == 0 and res >= 64, "three maps of stride 8 / 16 / 32"
    g = _NetGen(seed)
    g.tensor("image", 3, res, res, 1.0 / 127, 73.0)
    lk = dict(act=4, act_coef=0.1)
    x = g.conv("stem", "image", 16, 3, 1, 1, **lk)

    def stage(p, x, cout):
        d = g.conv(p + "_down", x, cout, 3, 2, 1, **lk)
        a = g.conv(p + "_a", d, cout // 2, 1, 1, 0, headroom=1.25, **lk)
        b = g.conv(p + "_b", a, cout, 3, 1, 1, **lk)
        return g.widen(g.add(p + "_res", d, b), 1.5)  # the sum of two leaky tensors has heavier tails than the sizing rule assumes

    x = stage("s2", stage("s1", x, 32), 48)
    m8 = stage("s3", x, 64)
    m16 = stage("s4", m8, 96)
    m32 = stage("s5", m16, 128)
    anchors = [int(round(a * res / 416.0)) or 1 for a in COCO_ANCHORS]
    ch = 3 * (5 + num_classes)
    boxes, scores = [], []

    def head(tag, f, k, ratio):
        hc = g.conv(tag + "_head", f, ch, 1, 1, 0, act=0, out_range=head_range)
        g.ops[-1]["bias"][4::5 + num_classes] -= np.float32(obj_shift * head_range)  # channel a * (5 + classes) + 4
        b, s = g.yolo_box([tag + "_boxes", tag + "_scores"], hc, "img_size", anchors[6 * k:6 * k + 6], num_classes, 0.01, ratio, True, 1.0)
        boxes.append(b)
        scores.append(s)

    p32 = g.conv("n32", m32, 64, 1, 1, 0, headroom=1.5, **lk)
    head("y32", p32, 2, 32)
    u = g.interp("n32_up", g.conv("n32_lat", p32, 32, 1, 1, 0, **lk), "nearest", (res // 16, res // 16), align_corners=False)
    p16 = g.conv("n16", g.widen(g.concat("n16_cat", [u, m16]), 1.25), 64, 3, 1, 1, headroom=1.5, **lk)
    head("y16", p16, 1, 16)
    u = g.interp("n16_up", g.conv("n16_lat", p16, 32, 1, 1, 0, **lk), "nearest", (res // 8, res // 8), align_corners=False)
    p8 = g.conv("n8", g.widen(g.concat("n8_cat", [u, m8]), 1.25), 64, 3, 1, 1, headroom=1.5, **lk)
    head("y8", p8, 0, 8)
    b = g.join("boxes", boxes, 1)
    s = g.transpose("scores", g.join("scores_npc", scores, 1), (0, 2, 1))
    det = g.multiclass_nms("det", b, s, -1, 0.01, 400, 0.45, 100, normalized=False)
    net = _finish(g, res, det)
    net["img_size"] = "img_size"
    return net


def concat_calib_bytes(net, batch):
    """Algorithmic bytes of every concat that a calib reads directly or through a max pool, as separate concat and calib
    instructions (17 per concatenated element: 4 + 4 for the move, 4 + 4 + 1 for the calib; counted where the calib reads the pool
    as if it read the concat) and as the one fused launch (9: the operands once, the int8 tensor once).  Counts, not measurements."""
    n = 0
    for o in net["ops"]:
        if o["op"] == "concat":
            c, h, w = net["shapes"][o["name"]]
            n += c * h * w * batch
    return 17 * n, 9 * n


def shuffle_unit_bytes(net, batch):
    """Algorithmic bytes of the data movement of every stride-1 unit tail (split, calib of the second half, concat, shuffle_channel)
    as separate instructions, and of the one fused launch: (53 h P, 13 h P) summed over the units, h the half width and P the
    plane.  Counts, not measurements."""
    sep = fused = 0
    for o in net["ops"]:
        if o["op"] == "split":
            c, h_, w_ = net["shapes"][o["names"][1]]
            sep += 53 * c * h_ * w_ * batch  # split 16, calib 5, concat 16, shuffle_channel 16
            fused += 13 * c * h_ * w_ * batch
    return sep, fused


def mobilenet_v1_net(seed=1234, res=224):
    """MobileNetV1 in op-list form, same weights as make_mobilenet_v1_weights(seed): graph mode must arrive at exactly
    the Appendix-D program that build_mobilenet_v1 writes out by hand."""
    W = make_mobilenet_v1_weights(seed, res)
    ops, shapes = [], {}
    cur = "image"
    for (name, op, cin, cout, k, s, p, g, hin) in mobilenet_v1_layers(res):
        L = W[name]
        ops.append(dict(op=op, name=name, src=cur, w=L["w"], bias=L["bias"], stride=s, pad=p, groups=g, act=1, act_coef=0.0,
                        in_scale=L["in_scale"], w_scale=L["w_scale"]))
        ho = (hin + 2 * p - k) // s + 1
        shapes[name] = (cout, ho, ho)
        cur = name
    ops.append(dict(op="pool2d", name="pool", src=cur, pooling_type="avg", ksize=shapes[cur][1], stride=1, pad=0,
                    global_pooling=True))
    shapes["pool"] = (shapes[cur][0], 1, 1)
    F = W["fc"]
    ops.append(dict(op="fc", name="logits", src="pool", w=F["w"], bias=F["bias"], in_scale=F["in_scale"], w_scale=F["w_scale"]))
    ops.append(dict(op="softmax", name="prob", src="logits"))
    shapes["logits"] = shapes["prob"] = (NUM_CLASSES, 1, 1)
    return dict(ops=ops, input="image", input_shape=(3, res, res), output="prob", shapes=shapes)


def net_stats(net):
    """MACs and algorithmic activation bytes per image by op class (int8 tensors 1 B/elt, fp32 tensors 4 B/elt are
    decided by the lowering; here: conv MACs and element counts only).  concat / split / shuffle_channel carry no MACs: their
    bytes are program_costs' and shuffle_unit_bytes'."""
    macs = {"conv1x1": 0, "conv_kxk": 0, "depthwise": 0, "fc": 0}
    shapes = net["shapes"]
    for o in net["ops"]:
        if o["op"] in ("conv2d", "depthwise_conv2d"):
            cout, cg, k, _ = o["w"].shape
            c, h, w = shapes[o["name"]]
            m = h * w * cout * cg * k * k
            key = "depthwise" if o["op"] == "depthwise_conv2d" else ("conv1x1" if k == 1 else "conv_kxk")
            macs[key] += m
        elif o["op"] == "fc":
            macs["fc"] += o["w"].shape[0] * o["w"].shape[1]
    return macs


def emit_graph(pred, net, batch, fuse=True, fuse_dwpw=None, fuse_dwconv=None, image=None, frame=None, fuse_hard_act=None, fuse_shuffle=None,
               fuse_concat=None, fuse_interp_argmax=None, fuse_interp_calib=None, fuse_detection_head=None, fetch=(), fuse_yolo_head=None):
    """Feed the op list to the predictor's graph mode and lower it.  Returns the host name of the output variable.
    image: None = the input is the normalised fp32 NCHW tensor; dict(format, means, scales) = the input is a decoded uint8 image
    [batch, h, w, cs] of that format (liteapi.IMG_*), normalised on the device (Predictor.graph_feed_image).
    frame: None = off; dict(h, w, format, means, scales) = the input is a frame batch of h x w in that format (liteapi.IMG_*, NV12 /
    NV21 included), converted, resized to the network's size and normalised on the device (Predictor.graph_feed_frame).
    fuse=False: the reference program instruction for instruction (no kHIP graph-level fusion).
    fuse_dwpw: None = the builder's default (depthwise -> pointwise pairs the fused kernel takes become one instruction),
    True = every eligible pair (shapes outside the kernel run as two launches inside the instruction), False = none.
    fuse_dwconv: None = the builder's default (off); True = fusion G, a depthwise conv takes its 1x1 consumer over together with
    that conv's fused tail (MobileNetV2's blocks), False = off.
    fuse_hard_act: None = the builder's default (off); True = fusions J1 / J2 / J3 of the MobileNetV3 ops (hard_swish and
    elementwise_mul take the calib behind them over, the excite chain becomes one hard_sigmoid/se_gate instruction).
    fuse_shuffle: None = the builder's default (on); fusion K of the ShuffleNetV2 ops (concat -> shuffle_channel(2) ->
    [split ->] calib becomes one shuffle_channel/unit or shuffle_channel/int8 instruction), False = the separate instructions.
    fuse_concat: None = the builder's default (on); fusion L of the fire / inception modules (a concat takes the calib that reads it
    over, concat/int8; a max pool behind it runs on the int8 copy), False = the separate instructions.
    fuse_interp_argmax / fuse_interp_calib: None = the builder's default (on); False = the separate instructions; fusions M (an interp whose only reader is
    arg_max(axis 1) becomes one arg_max/interp instruction) and N (an interp takes the calib that reads it over) of the dense
    prediction ops, each with a switch of its own.
    fuse_detection_head: None = the builder's default (on); False = the separate instructions; fusion O of the detection heads (a concat of transpose -> reshape
    chains becomes one concat/nhwc instruction; the transpose in front of multiclass_nms's scores disappears into its strides).
    fuse_yolo_head: None = the builder's default (on); fusion P of a YOLOv3 head (the yolo_box ops, the concats of their
    outputs and the transpose in front of multiclass_nms become one yolo_box/head instruction), False = the separate instructions.
    A net with an "img_size" entry gets that variable as a second feed, int32 [batch, 2] = (height, width) of every image.
    fetch: further variables to fetch beside net["output"] (host names: "<name>/host").  A multiclass_nms output is fetched together
    with its count variable "<name>/count"."""
    from . import liteapi
    pred.graph_set_fuse(fuse)
    if fuse_dwpw is not None:
        pred.graph_set_fuse_dwpw(fuse_dwpw)
    if fuse_dwconv is not None:
        pred.graph_set_fuse_dwconv(fuse_dwconv)
    if fuse_hard_act is not None:
        pred.graph_set_fuse_hard_act(fuse_hard_act)
    if fuse_shuffle is not None:
        pred.graph_set_fuse_shuffle(fuse_shuffle)
    if fuse_concat is not None:
        pred.graph_set_fuse_concat(fuse_concat)
    if fuse_interp_argmax is not None:
        pred.graph_set_fuse_interp_argmax(fuse_interp_argmax)
    if fuse_interp_calib is not None:
        pred.graph_set_fuse_interp_calib(fuse_interp_calib)
    if fuse_detection_head is not None:
        pred.graph_set_fuse_detection_head(fuse_detection_head)
    if fuse_yolo_head is not None:
        pred.graph_set_fuse_yolo_head(fuse_yolo_head)
    c, h, w = net["input_shape"]
    if frame is not None:
        assert image is None, "emit_graph: image= and frame= exclude each other"
        pred.graph_feed_frame(net["input"], batch, frame["h"], frame["w"], frame["format"], h, w, frame["means"], frame["scales"])
    elif image is None:
        pred.graph_feed(net["input"], (batch, c, h, w), liteapi.PREC_FLOAT)
    else:
        pred.graph_feed_image(net["input"], batch, h, w, image["format"], image["means"], image["scales"])
    if net.get("img_size"):
        pred.graph_feed(net["img_size"], (batch, 2), liteapi.PREC_INT32)
    for o in net["ops"]:
        t = o["op"]
        if t in ("conv2d", "depthwise_conv2d"):
            p = o["pad"]
            pred.graph_conv(t, o["src"], o["name"], o["w"], o["bias"], (o["stride"],) * 2, (p, p, p, p), (o.get("dilation", 1),) * 2, o["groups"],
                            o["act"], o["act_coef"], float(o["in_scale"]), o["w_scale"])
        elif t == "conv2d_transpose":
            p = o["pad"]
            pred.graph_conv2d_transpose(o["src"], o["name"], o["w"], o["bias"], (o["stride"],) * 2, (p, p, p, p), (o.get("dilation", 1),) * 2,
                                        o["groups"], o["act"], o["act_coef"], float(o["in_scale"]), o["w_scale"], o["output_size"])
        elif t == "fc":
            pred.graph_fc(o["src"], o["name"], o["w"], o["bias"], float(o["in_scale"]), o["w_scale"], False)
        elif t == "pool2d":
            p = o["pad"]
            pred.graph_pool(o["src"], o["name"], o["pooling_type"], (o["ksize"],) * 2, (o["stride"],) * 2, (p, p, p, p),
                            o["global_pooling"], True, False)
        elif t == "add":
            pred.graph_elementwise_add(o["x"], o["y"], o["name"], o["act"])
        elif t == "softmax":
            pred.graph_softmax(o["src"], o["name"])
        elif t == "hard_swish":
            pred.graph_hard_swish(o["src"], o["name"])
        elif t == "hard_sigmoid":
            pred.graph_hard_sigmoid(o["src"], o["name"])
        elif t == "mul":
            pred.graph_elementwise_mul(o["x"], o["y"], o["name"], 0)
        elif t == "concat":
            pred.graph_concat(o["srcs"], o["name"], o["axis"])
        elif t == "split":
            pred.graph_split(o["src"], o["names"], o["axis"], o["num"], o["sections"])
        elif t == "shuffle_channel":
            pred.graph_shuffle_channel(o["src"], o["name"], o["group"])
        elif t in ("bilinear_interp", "nearest_interp"):
            pred.graph_interp(t, o["src"], o["name"], (o["out_h"], o["out_w"]), 0.0, o["align_corners"], o["align_mode"])
        elif t == "arg_max":
            pred.graph_arg_max(o["src"], o["name"], o["axis"], o["dtype"], o["keepdims"])
        elif t == "transpose":
            pred.graph_transpose(o["src"], o["name"], o["perm"])
        elif t == "reshape":
            pred.graph_reshape(o["src"], o["name"], o["shape"])
        elif t == "prior_box":
            pred.graph_prior_box(o["src"], o["image"], o["names"][0], o["names"][1], o["min_sizes"], o["max_sizes"], o["aspect_ratios"],
                                 o["variances"], o["flip"], o["clip"], o["step_w"], o["step_h"], o["offset"], o["min_max_aspect_ratios_order"])
        elif t == "box_coder":
            pred.graph_box_coder(o["prior"], o["target"], o["name"], o["prior_var"], o["variance"], o["axis"], o["normalized"])
        elif t == "yolo_box":
            pred.graph_yolo_box(o["src"], o["img_size"], o["names"][0], o["names"][1], o["anchors"], o["class_num"], o["conf_thresh"],
                                o["downsample_ratio"], o["clip_bbox"], o["scale_x_y"])
        elif t == "multiclass_nms":
            pred.graph_multiclass_nms(o["boxes"], o["scores"], o["name"], o["background_label"], o["score_threshold"], o["nms_top_k"],
                                      o["nms_threshold"], o["nms_eta"], o["keep_top_k"], o["normalized"], o["index"])
        else:
            raise ValueError(t)
    for v in fetch:
        pred.graph_fetch(v)
    if net["ops"] and net["ops"][-1]["op"] == "multiclass_nms" and net["ops"][-1]["name"] == net["output"]:
        pred.graph_fetch(net["output"] + "/count")
    pred.graph_fetch(net["output"])
    return net["output"] + "/host"


def program_costs(net, batch, plan_lines):
    """Algorithmic work of every instruction of the lowered program (unique input + weights + output once,
    no im2col expansion, no re-reads), aligned with `plan_lines` (GraphBuilder::Plan / Predictor.graph_plan()).
    Returns [dict(name, family, ops, bytes)]; io_copy lines get family "io_copy" and zero cost."""
    shapes = dict(net["shapes"])
    shapes[net["input"]] = net["input_shape"]
    esz = {}  # variable -> bytes per element

    def numel(v):
        base = v.replace("/target_trans", "").replace("/precision_trans", "")
        c, h, w = shapes[base]
        return batch * c * h * w

    int8_ops = iter([o for o in net["ops"] if o["op"] in ("conv2d", "depthwise_conv2d", "fc")])  # never reordered
    out = []
    esz[net["input"]] = 4
    for line in plan_lines:
        head, rest = line.split(" ", 1)
        toks = rest.split(" ")
        kv = dict(f.split("=", 1) for f in toks if "=" in f)
        flags = {f for f in toks if "=" not in f}
        ins, dst = kv["in"].split(","), kv["out"]
        op, alias = head.split("/")
        if op in ("concat", "split") or op == "shuffle_channel":  # fp32 moves: every operand once, every written tensor once
            outs = dst.split(",")
            byts = sum(numel(i) * 4 for i in ins)
            if alias == "unit" and "+hi" in kv:  # (K1): the split's second half, where it has another reader
                outs.append(kv["+hi"])
            if "-f32" in flags:                  # (K2): the shuffled fp32 tensor is not written
                outs = []
            for v in outs:
                esz[v] = 4
                byts += numel(v) * 4
            for v in dst.split(","):
                esz.setdefault(v, 4)
            if "+calib" in kv:
                esz[kv["+calib"]] = 1
                byts += numel(kv["+calib"])
            fam = {"def": op, "unit": "shuffle_unit", "int8": "shuffle_concat"}[alias]
            out.append(dict(name=outs[0] if outs else kv["+calib"], family=fam, ops=0, bytes=byts))
            continue
        if op == "io_copy":
            esz[dst] = esz.get(ins[0], 4)
            out.append(dict(name=dst, family="io_copy", ops=0, bytes=0))
            continue
        if op == "calib":
            esz[dst] = 1 if alias == "fp32_to_int8" else 4
            out.append(dict(name=dst, family="calib", ops=0, bytes=numel(ins[0]) * esz[ins[0]] + numel(dst) * esz[dst]))
            continue
        if alias == "se_gate":  # (J2): the calib and the two 1x1 convs on 1 x 1 planes inside the hard_sigmoid instruction
            o1, o2 = next(int8_ops), next(int8_ops)
            esz[dst] = 4
            wb = int(o1["w"].size) + int(o2["w"].size)
            out.append(dict(name=dst, family="se_gate", ops=2 * batch * wb, bytes=numel(ins[0]) * 4 + wb + numel(dst) * 4))
            continue
        if op in ("conv2d", "depthwise_conv2d", "fc"):
            o = next(int8_ops)
            assert o["op"] == op, (o["op"], line)
            esz[dst] = 1 if alias in ("int8_out", "int8out") else 4
            wbytes = int(o["w"].size)
            if op == "fc":
                macs = batch * o["w"].shape[0] * o["w"].shape[1]
                fam = "fc"
            else:
                cout, cg, k, _ = o["w"].shape
                c, h, w = shapes[o["name"]]
                macs = batch * h * w * cout * cg * k * k
                cin = shapes[o["src"]][0]
                if op == "depthwise_conv2d":
                    fam = "depthwise%dx%d" % (k, k)
                elif k == 1:
                    fam = "pointwise1x1" if o["stride"] == 1 else "conv1x1s2"
                else:
                    fam = "stem_conv" if cin <= 4 else "conv%dx%d" % (k, k)
            byts = sum(numel(i) * esz[i] for i in ins) + wbytes
            if "+pw" in kv:       # opt-in fusion: this depthwise conv took its 1x1 consumer over: `dst` is that conv's output
                o2 = next(int8_ops)
                pw_name = kv.get("pw_out", dst)  # (+pool: `dst` is the global average pool's output, the conv's plane is never written)
                assert o2["op"] == "conv2d" and o2["name"] == pw_name, (o2["name"], line)
                esz[dst] = 1 if kv["+pw"].endswith("int8_out") else 4
                m2, c2 = o2["w"].shape[0], o2["w"].shape[1]
                _, h2, w2 = shapes[pw_name]
                macs += batch * h2 * w2 * m2 * c2
                wbytes += int(o2["w"].size)
                byts += int(o2["w"].size)
                fam = "dwpw_fused"
            if "-f32" not in flags:
                byts += numel(dst) * esz[dst]
            if "+add" in kv:      # fused residual operand (fp32)
                byts += numel(kv["+add"]) * 4
            if "+calib" in kv:    # fused int8 copy
                esz[kv["+calib"]] = 1
                byts += numel(kv["+calib"])
            out.append(dict(name=dst, family=fam, ops=2 * macs, bytes=byts))
        else:
            esz[dst] = 1 if "int8" in flags else 4
            fam = {"pool2d": "pool2d", "elementwise_add": "elementwise_add", "fusion_elementwise_add_activation": "elementwise_add",
                   "softmax": "softmax", "hard_swish": "hard_act", "hard_sigmoid": "hard_act", "elementwise_mul": "se_scale"}[op]
            byts = sum(numel(i) * esz[i] for i in ins) + (0 if "-f32" in flags else numel(dst) * esz[dst])
            if "+calib" in kv:    # (J1) (J3): the int8 copy of the same launch
                esz[kv["+calib"]] = 1
                byts += numel(kv["+calib"])
            out.append(dict(name=dst, family=fam, ops=0, bytes=byts))
    return out
