"""The grouped 3x3 route of the C ABI (conv_grouped_i8.hip) without a device: which descriptors it takes, what it leaves to the
route they had before, its packed-weight and workspace bytes, whole fixture lines for ResNeXt50's seven grouped shapes
(tests/golden/conv_routes/grouped.txt, `python tests/test_grouped_route_host.py` rewrites it) and the packed layout, restated in
numpy (test_gpu_grouped.py compares the device packer's bytes with this restatement)."""
import ctypes
import importlib.util
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_conv_routes", os.path.join(ROOT, "tools", "dump_conv_routes.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)

GROUPED = "conv_grouped3x3_int8_mfma32x32x32"
IM2COL = "conv_im2col_gemm_int8_mfma32x32x32"
GEMM_1X1 = "conv1x1s1_gemm_int8_mfma32x32x32"

# (cin, groups): every Cg in {4, 8, 16, 32}, groups 4 / 8 / 32 and others, cin 32 / 64 / 96 / 1024 and others
CIN_GROUPS = [(32, 4), (32, 8), (64, 4), (64, 8), (64, 16), (96, 6), (96, 12), (96, 24), (128, 4), (128, 32), (256, 32),
              (512, 32), (1024, 32), (1024, 64), (1024, 256)]
PADS = [(1, 1, 1, 1), (0, 0, 0, 0), (0, 1, 0, 1), (1, 0, 1, 0), (1, 1, 0, 0)]
# (n, cin, h, w, cout, kh, kw, pads, stride, dil, groups), as tests/edge_cases.ROUTES spells a shape
INSIDE = [(n, cin, h, w, cin, 3, 3, PADS[i % len(PADS)], st, 1, g)
          for i, ((cin, g), st, (n, h, w)) in enumerate(itertools.product(CIN_GROUPS, (1, 2), ((1, 7, 7), (3, 9, 13), (2, 56, 56))))]
# just outside the envelope: the route the descriptor had before
OUTSIDE = {
    "groups 2": ((2, 64, 14, 14, 64, 3, 3, (1,) * 4, 1, 1, 2), IM2COL),
    "Cg 2": ((2, 64, 14, 14, 64, 3, 3, (1,) * 4, 1, 1, 32), IM2COL),
    "Cg 64": ((2, 256, 14, 14, 256, 3, 3, (1,) * 4, 1, 1, 4), IM2COL),
    "Cg != Mg": ((2, 64, 14, 14, 128, 3, 3, (1,) * 4, 1, 1, 8), IM2COL),
    "cin 48, Cg 4": ((2, 48, 14, 14, 48, 3, 3, (1,) * 4, 1, 1, 12), IM2COL),
    "dilation 2": ((2, 64, 14, 14, 64, 3, 3, (1,) * 4, 1, 2, 8), IM2COL),
    "5x5": ((2, 64, 14, 14, 64, 5, 5, (1,) * 4, 1, 1, 8), IM2COL),
    "1x1 grouped": ((2, 64, 14, 14, 64, 1, 1, (0,) * 4, 1, 1, 8), GEMM_1X1),
    "padding 2": ((2, 64, 14, 14, 64, 3, 3, (2,) * 4, 1, 1, 8), IM2COL),
    "padding 2 on one side": ((2, 64, 14, 14, 64, 3, 3, (1, 1, 1, 2), 1, 1, 8), IM2COL),
    "stride 3": ((2, 64, 14, 14, 64, 3, 3, (1,) * 4, 3, 1, 8), IM2COL),
}
# ResNeXt50-32x4d's seven distinct grouped 3x3 shapes: (channels, input plane, stride)
RESNEXT_3X3 = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1)]


def _desc(capi, shape):
    n, cin, h, w, cout, kh, kw, pads, st, dl, g = shape
    if isinstance(st, int):
        st = (st, st)
    return capi.conv_desc(n, cin, h, w, cout, kh, kw, pads, st, (dl, dl), g, capi.ACT_RELU, 0.0)


def _answers(lib, d):
    r = ctypes.byref(d)
    return lib.plhip_conv_impl_name(r).decode(), lib.plhip_conv_packed_weight_bytes(r), lib.plhip_conv_workspace_bytes(r)


class _GroupedOff:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        assert self.lib.plhip_debug_set(b"CONV_GROUPED", 0) == 0

    def __exit__(self, *a):
        self.lib.plhip_debug_set(b"CONV_GROUPED", 1)


def _out_hw(shape):
    n, cin, h, w, cout, kh, kw, pads, st, dl, g = shape
    return int((h + pads[0] + pads[1] - 3) / st) + 1, int((w + pads[2] + pads[3] - 3) / st) + 1


def test_envelope_takes_the_grouped_route(pkg):
    capi, lib = pkg.capi, pkg.capi.load()
    assert {c // g for c, g in CIN_GROUPS} == {4, 8, 16, 32}
    assert {4, 8, 32} <= {g for _, g in CIN_GROUPS} and {32, 64, 96, 1024} <= {c for c, _ in CIN_GROUPS}
    assert {s[7] for s in INSIDE} == set(PADS) and {s[8] for s in INSIDE} == {1, 2}
    for shape in INSIDE:
        name, packed, ws = _answers(lib, _desc(capi, shape))
        assert name == GROUPED, shape
        assert packed == shape[1] // 32 * 9 * 1024, shape  # 9 A fragments of 1 KiB per 32-channel chunk
        assert ws == 0, shape                              # the kernel stages the input rows itself


def test_knob_off_is_the_im2col_route(pkg):
    """CONV_GROUPED = 0: the routing of the commit before the route existed; packed / workspace bytes by its formulas
    (gemm_packed_bytes, im2col_bytes in plhip_capi_conv.hip)."""
    capi, lib = pkg.capi, pkg.capi.load()
    with _GroupedOff(lib):
        for shape in INSIDE:
            n, cin, h, w, cout, kh, kw, pads, st, dl, g = shape
            name, packed, ws = _answers(lib, _desc(capi, shape))
            assert name == IM2COL, shape
            mg, kg = cout // g, cin // g * 9
            ma = 2 if mg > 32 else 1
            mt32 = -(-mg // (32 * ma)) * ma
            assert packed == g * mt32 * -(-kg // 32) * 1024, shape
            oh, ow = _out_hw(shape)
            assert ws == n * g * kg * (-(-(oh * ow) // 4) * 4), shape
    assert _answers(lib, _desc(capi, INSIDE[0]))[0] == GROUPED  # the knob is back


@pytest.mark.parametrize("what", sorted(OUTSIDE))
def test_outside_the_envelope_keeps_its_route(pkg, what):
    capi, lib = pkg.capi, pkg.capi.load()
    shape, want = OUTSIDE[what]
    got = _answers(lib, _desc(capi, shape))
    assert got[0] == want, (what, got)
    with _GroupedOff(lib):
        assert _answers(lib, _desc(capi, shape)) == got, what


def test_stride_2_by_1_keeps_its_route(pkg):
    capi, lib = pkg.capi, pkg.capi.load()
    d = _desc(capi, (2, 64, 14, 14, 64, 3, 3, (1,) * 4, (2, 1), 1, 8))
    assert _answers(lib, d)[0] == IM2COL


def resnext_shapes():
    return [((n, c, hw, hw, c, 3, 3, (1,) * 4, st, 1, 32), c) for n in dump.BATCHES for c, hw, st in RESNEXT_3X3]


def grouped_lines(pkg):
    ask = dump.Asker(pkg)
    return [ask.line(shape, m) for shape, m in resnext_shapes()]


def test_resnext_lines_equal_snapshot(pkg):
    got, want = grouped_lines(pkg), dump.load_fixture("grouped.txt")
    assert len(got) == len(want) == 21
    for g, w in zip(got, want):
        assert g == w, "the line differs\n  library : %s\n  recorded: %s" % (g, w)
        assert g.split(" | ")[1].split()[0] == GROUPED
    wl = importlib.import_module(pkg.__name__ + ".workloads")
    net = wl.resnext50_net()
    in_net = {s for s, _ in dump.net_shapes(net, 1) if s[10] == 32}
    assert in_net == {s for s, _ in resnext_shapes() if s[0] == 1}  # the seven shapes are the network's


# ---- the packed layout ------------------------------------------------------------------------------------------------------
def pack_index(cin, cg):
    """[cin / 32 chunks][9 taps][64 lanes][16 bytes] -> the flat OIHW index of the filter byte stored there, -1 = zero fill.
    Lane (m, h) byte j of tap t = r * 3 + s holds w[32 chunk + m][k % Cg][r][s] for the chunk's input channel k = 16 h + j when
    k and m are in the same group."""
    chunk, t, lane, j = np.meshgrid(np.arange(cin // 32), np.arange(9), np.arange(64), np.arange(16), indexing="ij")
    m, k = lane & 31, 16 * (lane >> 5) + j
    idx = ((chunk * 32 + m) * cg + k % cg) * 9 + t
    return np.where(m // cg == k // cg, idx, -1)


def pack_ref(w_oihw, cin, cg):
    idx = pack_index(cin, cg)
    flat = np.ascontiguousarray(w_oihw, np.int8).ravel()
    return np.where(idx >= 0, flat[np.maximum(idx, 0)], 0).astype(np.int8)


@pytest.mark.parametrize("cin,cg", [(32, 4), (64, 8), (96, 16), (128, 32), (96, 4)])
def test_packed_layout_places_every_filter_byte_once(cin, cg):
    idx = pack_index(cin, cg)
    assert idx.shape == (cin // 32, 9, 64, 16)
    used = np.sort(idx[idx >= 0])
    assert np.array_equal(used, np.arange(cin * cg * 9))  # every byte of the [cin, cg, 3, 3] filter, exactly once
    # what is stored sits on the diagonal blocks and carries the right (output channel, input channel, tap)
    chunk, t, lane, j = np.nonzero(idx >= 0)
    o, k = chunk * 32 + (lane & 31), chunk * 32 + 16 * (lane >> 5) + j
    assert np.array_equal(o // cg, k // cg)
    assert np.array_equal(idx[idx >= 0], (o * cg + k % cg) * 9 + t)
    assert (idx >= 0).sum() * 32 == idx.size * cg  # Cg / 32 of the fragment bytes are weights, the rest zero
    w = np.random.default_rng(cin + cg).integers(-127, 128, (cin, cg, 3, 3)).astype(np.int8)
    p = pack_ref(w, cin, cg)
    assert not p[idx < 0].any()
    assert p[0, 4, 33, 2] == (w[1, 18 % cg, 1, 1] if 1 // cg == 18 // cg else 0)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    with open(os.path.join(dump.ROUTES_DIR, "grouped.txt"), "w") as f:
        f.write("\n".join(grouped_lines(ge.import_package())) + "\n")
