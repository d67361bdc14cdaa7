"""The scale / bias / activation fold every kHIP kernel class shares (paddle-lite_amd/lite/kernels/hip/quant_fold.h), bit for bit.
A stand-alone program (its own main, g++ -fsanitize=address,undefined) includes the header, folds the cases below and prints the
result bits; the same values are computed here in numpy.float32, one operation at a time in the order the reference folds them
(conv_gemmlike.cc:208-263): ws * in_scale, then / out_scale; b / out_scale; relu6's coefficient / out_scale.  The int8 outputs
of every kernel are bit-exact against the oracle only in that order, so IN_SCALE / OUT_SCALE are chosen such that
ws * (in_scale / out_scale) rounds differently: a reordered fold cannot pass.  No device."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITE = os.path.join(ROOT, "paddle-lite_amd")
F = np.float32
OC = 5
IN_SCALE, OUT_SCALE = F(0.0314), F(0.0473)
WS = ((1 + np.arange(OC) % 7) / 127.0 / 4.0).astype(F)
BIAS = np.array([0.37, -1.25, 0.0, 2.0 / 3.0, -0.001], F)
NONE, RELU, RELU6, LEAKY = 0, 1, 2, 4  # lite_api::ActivationType == PLHIP_ACT_*
NO_PARAM = -1                          # the ActivationParam pointer is null (fc)

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <vector>
#include "lite/kernels/hip/quant_fold.h"
using namespace paddle::lite;
static float f32(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static std::vector<float> floats() {
  size_t n; std::cin >> n;
  std::vector<float> v(n);
  for (auto& x : v) { uint32_t u; std::cin >> std::hex >> u >> std::dec; x = f32(u); }
  return v;
}
// a case: oc int8_out fuse_relu act | in out coef (one hex word each) | n ws... | has_bias [n bias...]
int main() {
  int oc, int8_out, fuse_relu, act, has_bias;
  while (std::cin >> oc >> int8_out >> fuse_relu >> act) {
    uint32_t in, out, coef;
    std::cin >> std::hex >> in >> out >> coef >> std::dec;
    const std::vector<float> ws = floats();
    std::cin >> has_bias;
    std::vector<float> bias;
    if (has_bias) bias = floats();
    operators::ActivationParam ap;
    ap.has_active = act > 0;
    ap.active_type = static_cast<paddle::lite_api::ActivationType>(act > 0 ? act : 0);
    ap.Relu_clipped_coef = ap.Leaky_relu_alpha = f32(coef);
    try {
      const kernels::hip::QuantFold f = kernels::hip::FoldQuant(ws, oc, f32(in), f32(out), int8_out != 0, has_bias ? bias.data() : nullptr,
                                                                act < 0 ? nullptr : &ap, fuse_relu != 0);
      std::printf("%d %08x |", f.act, bits(f.alpha));
      for (float v : f.scale) std::printf(" %08x", bits(v));
      std::printf(" |");
      for (float v : f.bias) std::printf(" %08x", bits(v));
      std::printf("\n");
    } catch (const PaddleLiteException& e) {
      std::printf("FATAL %s\n", e.what());
    }
  }
  return 0;
}
"""


def _hex(a):
    return " ".join("%08x" % u for u in np.atleast_1d(np.asarray(a, F)).view(np.uint32))


def _case_line(c):
    line = "%d %d %d %d %s %s %s %d %s" % (c["oc"], c["int8_out"], c["fuse_relu"], c["act"], _hex(c["in"]), _hex(c["out"]), _hex(c["coef"]),
                                          len(c["ws"]), _hex(c["ws"]))
    return line + (" 1 %d %s" % (len(c["bias"]), _hex(c["bias"])) if c["bias"] is not None else " 0")


def _expected(c):
    """(act, alpha, scale, bias) in numpy.float32, one rounded operation per step."""
    ws = np.asarray(c["ws"], F)
    ws = np.full(c["oc"], ws[0], F) if ws.size == 1 else ws
    scale = ws * c["in"]
    if c["int8_out"]:
        scale = scale / c["out"]
    bias = None
    if c["bias"] is not None:
        bias = np.asarray(c["bias"], F) / c["out"] if c["int8_out"] else np.asarray(c["bias"], F)
    act = c["act"] if c["act"] > 0 else (RELU if c["fuse_relu"] else NONE)
    alpha = c["coef"] if act in (RELU6, LEAKY) else F(0)
    if act == RELU6 and c["int8_out"]:
        alpha = alpha / c["out"]
    return act, F(alpha), scale.astype(F), bias


def _cases():
    out = []
    for ws in (WS[:1], WS):                        # one scale broadcast to oc = 5 | oc scales
        for int8_out in (1, 0):
            for bias in (BIAS, None):
                for act, coef in ((NONE, 0.0), (RELU, 0.0), (RELU6, 6.0), (LEAKY, 0.2)):
                    out.append(dict(oc=OC, int8_out=int8_out, fuse_relu=0, act=act, coef=F(coef), ws=ws, bias=bias, **{"in": IN_SCALE, "out": OUT_SCALE}))
    base = dict(oc=OC, int8_out=1, coef=F(6.0), ws=WS, bias=BIAS, **{"in": IN_SCALE, "out": OUT_SCALE})
    out.append(dict(base, fuse_relu=1, act=NO_PARAM))      # the legacy flag without an ActivationParam
    out.append(dict(base, fuse_relu=0, act=NO_PARAM))      # fc: neither
    out.append(dict(base, fuse_relu=1, act=NONE))          # ... with a param that names no activation
    out.append(dict(base, fuse_relu=1, act=RELU6))         # the param wins over the flag; relu6's alpha with int8 output
    return out


@pytest.fixture(scope="module")
def folded():
    """[(case, output line)] of the stand-alone program over _cases() plus two that must end in LOG(FATAL)."""
    cases = _cases()
    bad = [dict(cases[0], ws=WS[:3]), dict(cases[0], act=5)]  # 3 scales for 5 channels; sigmoid cannot be fused
    with tempfile.TemporaryDirectory(prefix="quant_fold.") as tmp:
        src, exe = os.path.join(tmp, "fold_main.cc"), os.path.join(tmp, "fold_main")
        with open(src, "w") as f:
            f.write(PROGRAM)
        p = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", LITE,
                            "-I", os.path.join(ROOT, "include"), src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "quant_fold.h does not compile alone:\n" + p.stdout.decode()[-3000:]
        r = subprocess.run([exe], input="\n".join(_case_line(c) for c in cases + bad).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, "the sanitised fold failed:\n" + r.stderr.decode()[-3000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(cases) + len(bad), lines[-3:]
    return list(zip(cases, lines[:len(cases)])), lines[len(cases):]


def test_the_chosen_scales_tell_the_two_orders_apart():
    left = (WS * IN_SCALE / OUT_SCALE).view(np.uint32)
    regrouped = (WS * F(IN_SCALE / OUT_SCALE)).view(np.uint32)
    assert (left != regrouped).any(), "pick other scales: ws * in / out == ws * (in / out) for every entry"


def test_fold_is_bit_exact(folded):
    good, _ = folded
    assert len(good) == 2 * 2 * 2 * 4 + 4
    for c, line in good:
        act, alpha, scale, bias = _expected(c)
        head, s_bits, b_bits = [part.split() for part in line.split("|")]
        what = "ws=%d int8_out=%d bias=%s act=%d fuse_relu=%d: %s" % (len(c["ws"]), c["int8_out"], c["bias"] is not None, c["act"], c["fuse_relu"], line)
        assert int(head[0]) == act, what
        assert head[1] == _hex(alpha), what
        assert " ".join(s_bits) == _hex(scale) and len(s_bits) == c["oc"], what
        assert " ".join(b_bits) == (_hex(bias) if bias is not None else ""), what


def test_fold_refuses_what_the_reference_refuses(folded):
    _, bad = folded
    assert bad[0].startswith("FATAL") and bad[0].endswith("weights scale size must equal to filter size"), bad[0]
    assert bad[1].startswith("FATAL") and bad[1].endswith("this act_type: 5 fuse not support"), bad[1]
