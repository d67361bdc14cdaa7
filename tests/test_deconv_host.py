"""conv2d_transpose without a device: the numpy oracle (tests/deconv_oracle.py) against itself (scatter == gather), against
torch's conv_transpose2d in float64 and against accumulators minted from the reference's deconv_basic<int8_t, int>
(tests/golden/deconv_*.npz); the C ABI's route predicate, output dims and refusals; the packed layout of the phase route,
restated in numpy (test_gpu_deconv.py compares the device packer's bytes with this restatement); graph lowering (kernel pick, the
fusions that must not match, the plan fixtures of unet_mini_net, the unchanged plans of every existing workload); the plugin class
compiled against the reference's struct text; the structure and health of unet_mini_net on the CPU oracle."""
import ctypes
import glob
import importlib
import itertools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import deconv_oracle as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITE = os.path.join(ROOT, "paddle-lite_amd")
F32 = np.float32
PHASE = "deconv_phase_int8_mfma32x32x32"
DIRECT = "deconv_direct_int8"


def _operands(rng, n, cin, h, w, cout, kh, kw, groups):
    x = rng.integers(-128, 128, (n, cin, h, w)).astype(np.int8)
    wt = rng.integers(-128, 128, (cin, cout // groups, kh, kw)).astype(np.int8)
    return x, wt


# ---- 1. scatter == gather ---------------------------------------------------------------------------------------------------
PADS = ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 1, 0), (2, 0, 1, 2))
GROUPS = ((4, 6, 1), (4, 6, 2), (4, 4, 4))  # (cin, cout, groups): dense, two groups, depthwise


def _sweep():
    for k, s, dl in itertools.product(range(1, 6), range(1, 4), (1, 2)):
        for i, pads in enumerate(PADS):
            yield k, s, dl, pads, GROUPS[(k + s + dl + i) % 3]


def test_scatter_and_gather_forms_are_equal():
    rng = np.random.default_rng(11)
    seen = 0
    for k, s, dl, pads, (cin, cout, g) in _sweep():
        h, w = 3, 4
        kw = k if k % 2 else max(1, k - 1)  # a non-square filter on every other size
        try:
            oh, ow = D.out_dims(h, w, k, kw, pads, (s, s), (dl, dl))
        except ValueError:
            continue
        x, wt = _operands(rng, 2, cin, h, w, cout, k, kw, g)
        for extra in ((0, 0), (1, 0), (0, 1)):
            if s == 1 and extra != (0, 0):
                continue  # output_size + 1 needs a stride > 1
            osz = (oh + extra[0] if extra[0] else 0, ow + extra[1] if extra[1] else 0)
            a = D.acc_scatter(x, wt, pads, (s, s), (dl, dl), g, osz)
            b = D.acc_gather(x, wt, pads, (s, s), (dl, dl), g, osz)
            assert a.shape == (2, cout, oh + extra[0], ow + extra[1])
            assert np.array_equal(a, b), (k, kw, s, dl, pads, g, osz)
            seen += 1
    assert seen > 150
    # anisotropic strides and dilations
    x, wt = _operands(rng, 1, 4, 4, 3, 6, 3, 2, 2)
    assert np.array_equal(D.acc_scatter(x, wt, (1, 0, 0, 1), (2, 1), (1, 2), 2), D.acc_gather(x, wt, (1, 0, 0, 1), (2, 1), (1, 2), 2))


def test_output_size_outside_its_range_is_an_error():
    assert D.out_dims(4, 4, 3, 3, (1, 1, 1, 1), (2, 2), (1, 1)) == (7, 7)
    assert D.out_dims(4, 4, 3, 3, (1, 1, 1, 1), (2, 2), (1, 1), (8, 7)) == (8, 7)
    for bad in ((9, 0), (6, 0), (0, 9), (0, 6)):
        with pytest.raises(ValueError):
            D.out_dims(4, 4, 3, 3, (1, 1, 1, 1), (2, 2), (1, 1), bad)
    with pytest.raises(ValueError):
        D.out_dims(1, 1, 1, 1, (1, 0, 0, 0), (1, 1), (1, 1))


# ---- 2. torch in float64 on the same integers ---------------------------------------------------------------------------------
def test_oracle_equals_torch_conv_transpose2d():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(12)
    seen = 0
    for k, s, dl in itertools.product((1, 2, 3, 4, 5), (1, 2, 3), (1, 2)):
        for (ph, pw), (cin, cout, g) in zip(((0, 0), (1, 1), (2, 1)), GROUPS):
            try:
                oh, ow = D.out_dims(4, 5, k, k, (ph, ph, pw, pw), (s, s), (dl, dl))
            except ValueError:
                continue
            x, wt = _operands(rng, 2, cin, 4, 5, cout, k, k, g)
            for extra in ((0, 0), (1, 0), (0, 1), (1, 1)):
                if s == 1 and extra != (0, 0):
                    continue
                osz = (oh + extra[0] if extra[0] else 0, ow + extra[1] if extra[1] else 0)
                got = D.acc_gather(x, wt, (ph, ph, pw, pw), (s, s), (dl, dl), g, osz)
                want = F.conv_transpose2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(wt.astype(np.float64)), None,
                                          stride=s, padding=(ph, pw), output_padding=extra, groups=g, dilation=dl).numpy()
                assert got.shape == want.shape and np.array_equal(got.astype(np.float64), want), (k, s, dl, ph, pw, g, extra)
                seen += 1
    assert seen > 100


# ---- 3. the reference's own deconv_basic<int8_t, int> -------------------------------------------------------------------------
GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "deconv_*.npz")))


def test_golden_cases_are_the_six():
    assert [os.path.basename(p)[7:-4] for p in GOLDENS] == ["1x1", "depthwise", "g2_dil2", "k2s2", "k3s2_asym", "k4s2p1"]


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[7:-4])
def test_oracle_equals_the_reference_accumulators(path):
    z = np.load(path)
    assert "deconv_basic<int8_t, int>" in str(z["provenance"])
    args = (z["x"], z["w"], tuple(int(v) for v in z["pads"]), tuple(int(v) for v in z["strides"]), tuple(int(v) for v in z["dils"]),
            int(z["groups"]))
    assert z["acc"].dtype == np.int32 and z["acc"].any()
    assert np.array_equal(D.acc_scatter(*args), z["acc"])
    assert np.array_equal(D.acc_gather(*args), z["acc"])


# ---- 4. the route predicate ---------------------------------------------------------------------------------------------------
def _desc(capi, cin=32, cout=32, k=3, stride=(2, 2), pads=(1, 1, 1, 1), dil=(1, 1), groups=1, n=2, h=5, w=9, kw=None, osz=(0, 0)):
    return capi.deconv_desc(n, cin, h, w, cout, k, k if kw is None else kw, pads, stride, dil, groups, output_size=osz)


EDGES = [
    (dict(cin=31, cout=31), DIRECT), (dict(cin=32), PHASE), (dict(cin=33, cout=33), DIRECT), (dict(cin=64, cout=1), PHASE),
    (dict(k=4), PHASE), (dict(k=5), DIRECT), (dict(k=4, kw=5), DIRECT), (dict(k=1, pads=(0, 0, 0, 0)), PHASE),
    (dict(stride=(1, 1)), PHASE), (dict(stride=(2, 2)), PHASE), (dict(stride=(3, 3)), DIRECT), (dict(stride=(2, 1)), DIRECT),
    (dict(dil=(2, 2)), DIRECT), (dict(dil=(1, 2)), DIRECT), (dict(groups=2), DIRECT), (dict(groups=32), DIRECT),
    (dict(pads=(2, 2, 2, 2)), PHASE), (dict(pads=(3, 2, 2, 2), h=6), DIRECT), (dict(pads=(2, 2, 2, 3), w=6), DIRECT),
    (dict(osz=(10, 18)), PHASE),
]


@pytest.mark.parametrize("kw,want", EDGES, ids=[str(sorted(e[0].items())) for e in EDGES])
def test_route_on_the_envelope_edges(pkg, kw, want):
    capi = pkg.capi
    lib = capi.load()
    d = _desc(capi, **kw)
    assert capi.deconv_impl_name(d) == want
    c = d.conv
    filt = c.cin * (c.cout // c.groups) * c.kh * c.kw
    nbytes = lib.plhip_deconv_packed_weight_bytes(ctypes.byref(d))
    assert nbytes == (-(-c.cout // 32) * (c.cin // 32) * c.kh * c.kw * 1024 if want == PHASE else filt)
    # the knob forces the direct route for name and packed bytes alike, and goes back
    assert lib.plhip_debug_set(b"DECONV_ROUTE", 1) == 0
    try:
        assert capi.deconv_impl_name(d) == DIRECT and lib.plhip_deconv_packed_weight_bytes(ctypes.byref(d)) == filt
    finally:
        lib.plhip_debug_set(b"DECONV_ROUTE", 0)
    assert capi.deconv_impl_name(d) == want


# ---- 5. output dims and refusals ------------------------------------------------------------------------------------------------
def test_out_dims_follow_the_oracle(pkg):
    capi = pkg.capi
    for k, s, dl, pads in itertools.product((1, 2, 3, 4, 5), (1, 2, 3), (1, 2), PADS):
        d = capi.deconv_desc(1, 4, 5, 7, 4, k, k, pads, (s, s), (dl, dl))
        try:
            want = D.out_dims(5, 7, k, k, pads, (s, s), (dl, dl))
        except ValueError:
            with pytest.raises(capi.PlhipError, match="non-positive output"):
                capi.deconv_out_hw(d)
            continue
        assert capi.deconv_out_hw(d) == want
        for eh, ew in ((s - 1, 0), (0, s - 1)):
            d2 = capi.deconv_desc(1, 4, 5, 7, 4, k, k, pads, (s, s), (dl, dl), output_size=(want[0] + eh, want[1] + ew))
            assert capi.deconv_out_hw(d2) == (want[0] + eh, want[1] + ew)
    d = capi.deconv_desc(1, 4, 5, 7, 4, 3, 3, (1, 1, 1, 1), (2, 1))
    assert capi.deconv_out_hw(d) == (9, 7)


BAD = {
    "output_size one too large": dict(k=3, osz=(11, 0)),
    "output_size below the default": dict(k=3, osz=(0, 16)),
    "output_size negative": dict(k=3, osz=(-1, 0)),
    "cin % groups": dict(cin=33, cout=32, groups=2),
    "cout % groups": dict(cin=32, cout=33, groups=2),
    "non-positive output": dict(k=1, pads=(5, 5, 0, 0), stride=(1, 1)),
    "zero stride": dict(stride=(0, 1)),
    "zero dilation": dict(dil=(1, 0)),
    "negative padding": dict(pads=(0, -1, 0, 0)),
    "zero channels": dict(cin=0),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_bad_descriptors_are_invalid(pkg, what):
    capi = pkg.capi
    lib = capi.load()
    d = _desc(capi, **BAD[what])
    oh, ow = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.plhip_deconv_out_dims(ctypes.byref(d), ctypes.byref(oh), ctypes.byref(ow)) == -1  # PLHIP_ERR_INVALID
    assert (oh.value, ow.value) == (-7, -7)
    assert lib.plhip_last_error(None).decode().startswith("plhip_deconv_out_dims: ")
    assert capi.deconv_impl_name(d) == "invalid"
    assert lib.plhip_deconv_packed_weight_bytes(ctypes.byref(d)) == 0


def test_null_arguments_are_refused_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    d = _desc(capi)
    assert lib.plhip_deconv_out_dims(None, None, None) == -1
    assert lib.plhip_pack_deconv_weights(None, ctypes.byref(d), None, None) == -1
    assert lib.plhip_conv2d_transpose_int8(None, ctypes.byref(d), None, None, None, None, None, capi.OUT_I8) == -1
    assert "plhip_conv2d_transpose_int8: null argument" in lib.plhip_last_error(None).decode()
    assert ctypes.sizeof(capi.DeconvDesc) == ctypes.sizeof(capi.ConvDesc) + 8


# ---- the packed layout of the phase route ---------------------------------------------------------------------------------------
def pack_index(cin, cout, kh, kw):
    """[ceil(cout / 32) M tiles][cin / 32 chunks][kh * kw taps][64 lanes][16 bytes] -> the flat index into the [cin][cout][kh][kw]
    filter of the byte stored there, -1 = zero fill.  Lane (m, h) byte j of tap t = r * kw + s holds
    w[32 chunk + 16 h + j][32 tile + m][r][s]."""
    mt, chunk, t, lane, j = np.meshgrid(np.arange(-(-cout // 32)), np.arange(cin // 32), np.arange(kh * kw), np.arange(64),
                                        np.arange(16), indexing="ij")
    m, k = mt * 32 + (lane & 31), chunk * 32 + 16 * (lane >> 5) + j
    return np.where(m < cout, (k * cout + np.minimum(m, cout - 1)) * (kh * kw) + t, -1)


def pack_ref(w_iohw, cin, cout, kh, kw):
    idx = pack_index(cin, cout, kh, kw)
    flat = np.ascontiguousarray(w_iohw, np.int8).ravel()
    return np.where(idx >= 0, flat[np.maximum(idx, 0)], 0).astype(np.int8)


@pytest.mark.parametrize("cin,cout,kh,kw", [(32, 32, 2, 2), (64, 21, 3, 3), (96, 33, 4, 4), (32, 1, 1, 1), (64, 64, 4, 2)])
def test_packed_layout_places_every_filter_byte_once(cin, cout, kh, kw):
    idx = pack_index(cin, cout, kh, kw)
    assert idx.shape == (-(-cout // 32), cin // 32, kh * kw, 64, 16)
    assert np.array_equal(np.sort(idx[idx >= 0]), np.arange(cin * cout * kh * kw))
    w = np.random.default_rng(cin + cout).integers(-128, 128, (cin, cout, kh, kw)).astype(np.int8)
    p = pack_ref(w, cin, cout, kh, kw)
    assert not p[idx < 0].any()
    assert p[0, 0, kh * kw - 1, 32, 3] == w[19, 0, kh - 1, kw - 1]  # lane (m 0, h 1) byte 3: input channel 16 + 3


# ---- 6. graph lowering ------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def lite(pkg):
    return importlib.import_module("paddle_lite_amd.liteapi")


@pytest.fixture(scope="module")
def wl(pkg):
    return importlib.import_module("paddle_lite_amd.workloads")


@pytest.fixture(scope="module")
def unet(wl):
    return wl.unet_mini_net()


def _heads(plan):
    return [l.split(" ")[0] for l in plan]


def test_plugin_symbols_are_exported_and_the_kernels_registered(pkg, lite):
    capi = pkg.capi
    L, LL = capi.load(), lite.load()
    for name in ("plhip_deconv_out_dims", "plhip_deconv_packed_weight_bytes", "plhip_pack_deconv_weights", "plhip_conv2d_transpose_int8",
                 "plhip_deconv_impl_name"):
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert "DECONV_ROUTE" in capi.KNOBS and hasattr(capi.Context, "conv2d_transpose")
    assert hasattr(LL, "pllite_graph_conv2d_transpose") and hasattr(lite.Predictor, "graph_conv2d_transpose")
    assert LL.pllite_registered_kernels(b"conv2d_transpose", lite.PREC_INT8, lite.LAYOUT_NCHW) == 2
    src = open(os.path.join(LITE, "lite", "kernels", "hip", "deconv_compute.cc")).read()
    assert re.findall(r"REGISTER_LITE_KERNEL\((\w+), kHIP, (\w+), (\w+), [\w:]+, (\w+)\)", src) == [
        ("conv2d_transpose", "kInt8", "kNCHW", "int8_out"), ("conv2d_transpose", "kInt8", "kNCHW", "fp32_out")]


def test_unet_plans_equal_the_fixtures_and_the_oracles_plan(pkg, unet):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dump_deconv_plans as T
    golden = T.load_fixtures()
    assert sorted(golden) == ["unet_mini.default.b2", "unet_mini.nofuse.b2"]
    got = T.plans(pkg)
    for name in golden:
        assert got[name] == golden[name], name
    nofuse, default = golden["unet_mini.nofuse.b2"], golden["unet_mini.default.b2"]
    # the unfused program against the oracle's plan: every calib and every kernel pick
    want = D.plan(unet)
    body = nofuse[1:-1]
    assert len(body) == len(want)
    for line, (kind, s) in zip(body, want):
        head, toks = line.split(" ")[0], line.split(" ")
        if kind == "calib":
            src = s["src"] + ("/target_trans" if s["src"] == unet["input"] else "")
            assert head == "calib/fp32_to_int8" and ("in=" + src) in toks and ("out=" + s["dst"]) in toks, line
            continue
        o = s["o"]
        alias = ("int8_out" if s["int8_out"] else "fp32_out") if o["op"] in D.INT8_OPS else "def"
        assert head == o["op"] + "/" + alias and ("in=" + ",".join(s["ins"])) in toks and ("out=" + o["name"]) in toks, line
    # both transposed convs read an int8 tensor and write fp32 (a concat reads them); no rewrite hands them a tail or a front
    for plan in (nofuse, default):
        lines = [l for l in plan if l.startswith("conv2d_transpose")]
        assert lines == ["conv2d_transpose/fp32_out in=bottleneck out=dec2_up", "conv2d_transpose/fp32_out in=dec2_conv out=dec1_up"]
    # fusion L takes both concats with the fp32 outputs of the transposed convs as operands
    assert _heads(default).count("concat/int8") == 2 and len(nofuse) - len(default) == 2
    assert "concat/int8 in=dec2_up,enc2_conv out=dec2_concat +calib=dec2_concat/precision_trans scale=0.0314960629 -f32 axis=1" in default


def _planner(lite):
    return lite.Predictor(planner=True)


def _deconv_graph(lite, reader, k=3, stride=2, pad=1, output_size=None, cin=32, cout=32, w_shape=None, fetch_up=False):
    """feed -> conv2d 1x1 -> conv2d_transpose -> `reader`; returns the plan."""
    p = _planner(lite)
    try:
        p.graph_feed("x", (2, cin, 5, 7), lite.PREC_FLOAT)
        ones = np.ones(cin, F32)
        p.graph_conv("conv2d", "x", "a", np.ones((cin, cin, 1, 1), np.int8), None, (1, 1), (0, 0, 0, 0), (1, 1), 1, 1, 0.0, 0.01, ones)
        w = np.ones(w_shape or (cin, cout, k, k), np.int8)
        p.graph_conv2d_transpose("a", "up", w, np.zeros(cout, F32), (stride, stride), (pad, pad), (1, 1), 1, 1, 0.0, 0.02, np.ones(cout, F32),
                                 output_size)
        if reader == "conv":      # an int8 reader: int8_out at the reader's input scale
            p.graph_conv("conv2d", "up", "y", np.ones((8, cout, 1, 1), np.int8), None, (1, 1), (0, 0, 0, 0), (1, 1), 1, 0, 0.0, 0.25, np.ones(8, F32))
        elif reader == "add":     # conv2d[fp32_out] -> elementwise_add -> calib would be fusion A on a conv2d
            p.graph_conv("conv2d", "x", "side", np.ones((cout, cin, 1, 1), np.int8), None, (2, 2), (0, 0, 0, 0), (1, 1), 1, 0, 0.0, 0.01, np.ones(cout, F32))
            p.graph_elementwise_add("up", "up", "sum")
            p.graph_conv("conv2d", "sum", "y", np.ones((8, cout, 1, 1), np.int8), None, (1, 1), (0, 0, 0, 0), (1, 1), 1, 0, 0.0, 0.25, np.ones(8, F32))
        elif reader == "pool":    # conv2d[fp32_out] -> pool2d(max) -> calib would be fusion C on a conv2d
            p.graph_pool("up", "pooled", "max", (2, 2), (2, 2), (0, 0, 0, 0))
            p.graph_conv("conv2d", "pooled", "y", np.ones((8, cout, 1, 1), np.int8), None, (1, 1), (0, 0, 0, 0), (1, 1), 1, 0, 0.0, 0.25, np.ones(8, F32))
        if fetch_up:
            p.graph_fetch("up")
        p.graph_fetch("y" if reader else "up")
        return p.graph_plan()
    finally:
        p.close()


def test_kernel_pick_and_the_fusions_that_must_not_match(lite):
    plan = _deconv_graph(lite, "conv")
    assert "conv2d_transpose/int8_out in=a out=up oscale=0.25" in plan            # every reader int8: the reader's input scale
    assert "conv2d/int8_out in=x/precision_trans out=a oscale=0.0199999996" in plan  # and it is an int8 reader itself
    plan = _deconv_graph(lite, "conv", fetch_up=True)
    assert "conv2d_transpose/fp32_out in=a out=up" in plan and "calib/fp32_to_int8 in=up out=up/precision_trans scale=0.25" in plan
    plan = _deconv_graph(lite, "add")   # A / B: an fp32 conv2d would take the add and the calib over
    assert "conv2d_transpose/fp32_out in=a out=up" in plan and "elementwise_add/def in=up,up out=sum" in plan
    plan = _deconv_graph(lite, "pool")  # C: an fp32 conv2d would take the calib over and the pool would run on int8
    assert "conv2d_transpose/fp32_out in=a out=up" in plan and "pool2d/def in=up out=pooled" in plan
    assert "calib/fp32_to_int8 in=pooled out=pooled/precision_trans scale=0.25" in plan
    plan = _deconv_graph(lite, "conv", output_size=(10, 13))
    assert "conv2d_transpose/int8_out in=a out=up output_size=10x13 oscale=0.25" in plan


@pytest.mark.parametrize("kw,msg", [
    (dict(output_size=(11, 13)), "output_size 11 outside"), (dict(output_size=(9, 12)), "output_size 12 outside"),
    (dict(w_shape=(16, 32, 3, 3)), "the filter's first extent 16"), (dict(k=1, pad=5), "is empty")])
def test_graph_refuses_what_the_kernel_is_fatal_on(lite, kw, msg):
    with pytest.raises(Exception, match=msg):
        _deconv_graph(lite, "conv", **kw)


def test_no_plan_of_an_existing_workload_changes(pkg):
    """Every plan fixture of the existing workloads is regenerated and found unchanged."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    for tool in ("dump_plans", "dump_concat_plans", "dump_interp_plans", "dump_detection_plans"):
        t = importlib.import_module(tool)
        golden, got = t.load_fixtures(), t.plans(pkg)
        assert sorted(golden) == sorted(got) and golden, tool
        for name in golden:
            assert got[name] == golden[name], (tool, name)


# ---- 7. the plugin class against the reference's struct text ------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir("/root/reference/lite"), reason="reference tree not present on this machine")
def test_deconv_compute_compiles_against_the_reference_param_structs():
    """The method of test_detection_plugin_host.py: the generated header holds the reference's own ConvParam text (output_size among
    its fields), and deconv_compute.cc reads nothing else."""
    with tempfile.TemporaryDirectory(prefix="khip_refparams.") as tmp:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_ref_params_header.py"), "--out", tmp], stdout=subprocess.DEVNULL)
        gen = open(os.path.join(tmp, "lite", "operators", "op_params.h")).read()
        conv = re.search(r"struct ConvParam.*?\n};", gen, re.S).group(0)
        assert "std::vector<int> output_size" in conv
        p = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", tmp, "-I", LITE, "-I", os.path.join(ROOT, "include"),
                            os.path.join(LITE, "lite", "kernels", "hip", "deconv_compute.cc")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "deconv_compute.cc does not compile against the reference's structs:\n%s" % p.stdout.decode()[-3000:]


def test_op_infer_shape_follows_the_oracle(lite):
    """ConvTransposeOpLite::InferShape through a lowered planner graph is not reachable without a device; the shape rule is checked
    where the planner uses it (GraphBuilder::InferShapes) against deconv_oracle.out_dims: a wrong extent would move the int8 reader's
    plan line, and an output_size one past the range is refused (test_graph_refuses_what_the_kernel_is_fatal_on)."""
    for k, s, pad in ((2, 2, 0), (4, 2, 1), (3, 2, 1), (3, 1, 1), (1, 1, 0)):
        oh, ow = D.out_dims(5, 7, k, k, (pad,) * 4, (s, s), (1, 1))
        plan = _deconv_graph(lite, "conv", k=k, stride=s, pad=pad, output_size=(oh, ow))
        assert "output_size=%dx%d" % (oh, ow) in " ".join(plan)
        if s > 1:
            with pytest.raises(Exception, match="outside"):
                _deconv_graph(lite, "conv", k=k, stride=s, pad=pad, output_size=(oh + s, ow))


# ---- the U-Net: structure and health, on the oracle alone ---------------------------------------------------------------------------
def test_structure_of_unet_mini_net(wl, unet):
    ops, sh = unet["ops"], unet["shapes"]
    assert unet["input_shape"] == (3, 64, 64) and unet["output"] == "label" and sh["label"] == (64, 64)
    assert sh["enc1_conv2"] == (32, 64, 64) and sh["enc2_conv"] == (64, 32, 32) and sh["bottleneck"] == (128, 16, 16)
    assert sh["dec2_up"] == (64, 32, 32) and sh["dec2_concat"] == (128, 32, 32) and sh["dec1_up"] == (32, 64, 64) and sh["dec1_concat"] == (64, 64, 64)
    assert sh["logits"] == (4, 64, 64)
    by = {o["name"]: o for o in ops}
    up2, up1 = by["dec2_up"], by["dec1_up"]
    assert (up2["op"], up2["w"].shape, up2["stride"], up2["pad"]) == ("conv2d_transpose", (128, 64, 2, 2), 2, 0)
    assert (up1["op"], up1["w"].shape, up1["stride"], up1["pad"]) == ("conv2d_transpose", (64, 32, 4, 4), 2, 1)
    assert up2["bias"].shape == (64,) and up1["w_scale"].shape == (32,) and up1["output_size"] is None
    assert by["dec2_concat"]["srcs"] == ["dec2_up", "enc2_conv"] and by["dec1_concat"]["srcs"] == ["dec1_up", "enc1_conv2"]
    assert by["logits"]["act"] == 0 and by["logits"]["w"].shape == (4, 32, 1, 1)
    assert [o["op"] for o in ops].count("pool2d") == 2 and ops[-1]["op"] == "arg_max"
    big = wl.unet_mini_net(res=96)["shapes"]
    assert big["bottleneck"] == (128, 24, 24) and big["dec1_up"] == (32, 96, 96)


def test_unet_mini_net_is_as_healthy_as_mobilenet_v2(pkg, wl, plref, unet):
    """The rule of test_squeezenet_host.py: the yardstick is computed here from the worst int8 tensor of mobilenet_v2_net on images of
    the same seed (0.048 saturated, 0.637 zeros when this was written).  Measured on the committed seed: the worst saturated share is
    0.031 (the first pooled tensor), the worst zero share 0.572 (dec1_conv), over 9 int8 tensors.  Both transposed convs take the MFMA
    phase route at the network's shapes, and no pixel's two largest logits are within 1e-5 of each other."""
    import oracle.graph_oracle as GO
    capi = pkg.capi
    img = np.random.default_rng(350).uniform(-1, 1, (2, 3, 224, 224)).astype(F32)
    mb = {k: v for k, v in GO.forward(plref, wl.mobilenet_v2_net(), img, via_gemm=True).items() if v.dtype == np.int8}
    worst_sat = max((np.abs(v.astype(np.int32)) == 127).mean() for v in mb.values())
    worst_zero = max((v == 0).mean() for v in mb.values())
    assert 0 < worst_sat < 0.1 and 0.5 < worst_zero < 0.8
    img64 = np.random.default_rng(350).uniform(-1, 1, (2, 3, 64, 64)).astype(F32)
    ref = D.forward(plref, unet, img64)
    sh = {k: ((np.abs(v.astype(np.int32)) == 127).mean(), (v == 0).mean()) for k, v in ref.items() if v.dtype == np.int8}
    assert len(sh) == 9, sorted(sh)
    print("unet_mini: worst saturated %.4f (yardstick %.4f), worst zero %.4f (yardstick %.4f)" % (
        max(v[0] for v in sh.values()), worst_sat, max(v[1] for v in sh.values()), worst_zero))
    for name, (sat, zero) in sh.items():
        assert sat <= worst_sat, (name, sat, worst_sat)
        assert zero <= worst_zero, (name, zero, worst_zero)
    label, logits = ref["label"], ref["logits"]
    assert label.shape == (2, 64, 64) and label.dtype == np.int64 and set(np.unique(label)) == {0, 1, 2, 3}
    top = np.sort(logits, axis=1)
    close = (top[:, -1] - top[:, -2]) < 1e-5
    print("unet_mini: %d of %d pixels have their two largest logits within 1e-5" % (close.sum(), close.size))
    assert close.sum() == 0
    for name in ("dec2_up", "dec1_up"):
        o = next(q for q in unet["ops"] if q["name"] == name)
        cin, h, w = unet["shapes"][o["src"]]
        d = capi.deconv_desc(2, cin, h, w, o["w"].shape[1], o["w"].shape[2], o["w"].shape[3], (o["pad"],) * 4, (o["stride"],) * 2)
        assert capi.deconv_impl_name(d) == PHASE and capi.deconv_out_hw(d) == unet["shapes"][name][1:]
