"""-m gpu: the glue kernels every program runs (calib both ways, elementwise_add, pool2d fp32 / int8, global_avg_pool, softmax,
the fc launcher's three kernels) at their alignment, grid and value edges, against the numpy / float64 references of
glue_cases.py and the C oracle.

Every output lies in the middle of a larger allocation whose 64 bytes on either side hold a poison byte: the whole allocation
is read back and the bands must be untouched.  Inputs have the same margins (zeroed), so no case depends on what lies past an
allocation's end: a bad write shows in a band, a bad read in a wrong value."""
import ctypes as C
import importlib

import numpy as np
import pytest

import glue_cases as G
import mbv3_oracle as M

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD, POISON = 64, 0xA5


class _Dev:
    """The buffers of one device scope, each with GUARD bytes on either side, `off` bytes past a 16-byte boundary."""

    def __init__(self, ctx):
        self.ctx, self.scope = ctx, ctx.scope()

    def put(self, arr, off=0):
        """An input: zeroed margins, the array `off` bytes past a 16-byte boundary."""
        arr = np.ascontiguousarray(arr)
        p = self.scope.out(arr.shape, arr.dtype, off, fill=0, guard=GUARD).ptr
        self.ctx.check(self.ctx.L.plhip_memcpy_h2d(self.ctx.h, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "h2d")
        return p

    def out(self, shape, dtype, off=0):
        """A guarded output: (pointer, fetch); fetch() reads the margins back, checks both bands and returns the array."""
        o = self.scope.out(shape, dtype, off, fill=POISON, guard=GUARD)

        def fetch(what=""):
            around = o.margins()
            lo, hi = around[:GUARD + off], around[GUARD + off:]
            assert (lo == POISON).all(), "%s: %d bytes written before the output" % (what, (lo != POISON).sum())
            assert (hi == POISON).all(), "%s: %d bytes written past the output" % (what, (hi != POISON).sum())
            return o.get()
        return o.ptr, fetch

    def release(self):
        self.scope.release()


@pytest.fixture
def dev(gpu_ctx):
    d = _Dev(gpu_ctx)
    yield d
    d.release()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, "%s: %d of %d fp32 values differ, first at %d: got %r want %r" % (
        what, bad.size, g.size, bad[0], got.ravel()[bad[0]], np.asarray(want).ravel()[bad[0]])


def _same_i8(got, want, what):
    bad = np.flatnonzero(got.ravel() != np.asarray(want).ravel())
    assert bad.size == 0, "%s: %d of %d int8 values differ, first at %d: got %d want %d" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], np.asarray(want).ravel()[bad[0]])


# ------------------------------------------------------------------ 1. calib both ways, elementwise_add
def _calib_f2i(dev, x, scale, xo, yo, what):
    ctx = dev.ctx
    px = dev.put(x, xo)
    py, fetch = dev.out(x.shape, np.int8, yo)
    ctx.check(ctx.L.plhip_calib_f32_to_i8(ctx.h, px, py, float(scale), x.size), "calib_f32_to_i8")
    got = fetch(what)
    dev.release()
    return got


def _calib_i2f(dev, q, scale, xo, yo, what):
    ctx = dev.ctx
    px = dev.put(q, xo)
    py, fetch = dev.out(q.shape, F32, yo)
    ctx.check(ctx.L.plhip_calib_i8_to_f32(ctx.h, px, py, float(scale), q.size), "calib_i8_to_f32")
    got = fetch(what)
    dev.release()
    return got


def _add(dev, x, y, relu, xo, yo, oo, what):
    ctx = dev.ctx
    px, py = dev.put(x, xo), dev.put(y, yo)
    po, fetch = dev.out(x.shape, F32, oo)
    ctx.check(ctx.L.plhip_elementwise_add_f32(ctx.h, px, py, po, x.size, int(relu)), "elementwise_add")
    got = fetch(what)
    dev.release()
    return got


@pytest.mark.parametrize("scale", G.CALIB_SCALES)
def test_calib_f32_to_i8_alignments_and_ties(dev, scale):
    """Every count x (fp32 base off by 0 / 1 element) x (int8 base off by 0..3 bytes): the vector path only when both allow
    it, the scalar loop otherwise, an output misaligned alone included.  Values: exact ties of both signs, the bounds, past
    them, +-inf, +-0.  Bit for bit against round-half-away of fl32(x * fl32(1 / scale)); never -128."""
    paths, seed = set(), 0
    for count in G.COUNTS:
        for xo in (0, 4):
            for yo in (0, 1, 2, 3):
                seed += 1
                x = G.calib_f2i_input(scale, count, seed)
                what = "calib f32->i8 scale %g count %d x+%d y+%d" % (scale, count, xo, yo)
                got = _calib_f2i(dev, x, scale, xo, yo, what)
                _same_i8(got, G.calib_i8(x, scale), what)
                _same_i8(got, M.calib_i8(x, scale), what + " (mbv3_oracle)")
                assert got.min() >= -127, what
                paths.add(G.calib_f2i_vec(xo, yo))
    assert paths == {True, False}
    # the whole edge list in one aligned and one misaligned launch
    x = G.calib_edge_values(scale)
    for xo, yo in ((0, 0), (4, 0), (0, 1)):
        got = _calib_f2i(dev, x, scale, xo, yo, "edge list")
        _same_i8(got, G.calib_i8(x, scale), "calib edge list scale %g x+%d y+%d" % (scale, xo, yo))
        assert got.min() == -127 and got.max() == 127


@pytest.mark.parametrize("scale", [2.0 ** -4, 12.0 / 127])
def test_calib_i8_to_f32_alignments(dev, scale):
    """Every count x (int8 base off by 0..3 bytes) x (fp32 base off by 0 / 1 element), every int8 value, -128 included: q * scale,
    one fp32 multiply, bit for bit."""
    paths, seed = set(), 0
    for count in G.COUNTS:
        for xo in (0, 1, 2, 3):
            for yo in (0, 4):
                seed += 1
                q = G.calib_i2f_input(count, seed)
                what = "calib i8->f32 scale %g count %d x+%d y+%d" % (scale, count, xo, yo)
                _same_bits(_calib_i2f(dev, q, scale, xo, yo, what), G.calib_f32(q, scale), what)
                paths.add(G.calib_i2f_vec(xo, yo))
    assert paths == {True, False}


@pytest.mark.parametrize("relu", [False, True])
def test_elementwise_add_alignments_and_signed_zeros(dev, relu):
    """Every count x each of the three bases off by 0 / 1 element independently; +-0 in every pairing (relu(-0.0) is +0.0),
    FLT_MAX + FLT_MAX, inf + finite, exact cancellation.  Bit for bit against x + y, then r > 0 ? r : 0."""
    paths, seed = set(), 0
    for count in G.COUNTS:
        for xo in (0, 4):
            for yo in (0, 4):
                for oo in (0, 4):
                    seed += 1
                    x, y = G.add_input(count, seed)
                    what = "add relu %d count %d x+%d y+%d o+%d" % (relu, count, xo, yo, oo)
                    _same_bits(_add(dev, x, y, relu, xo, yo, oo, what), G.add_ref(x, y, relu), what)
                    paths.add(G.add_vec(xo, yo, oo))
    assert paths == {True, False}
    ex, ey = G.add_edge_pairs()
    for offs in ((0, 0, 0), (0, 0, 4)):
        _same_bits(_add(dev, ex, ey, relu, *offs, "add edge pairs"), G.add_ref(ex, ey, relu), "add edge pairs relu %d offsets %r" % (relu, offs))


@pytest.mark.parametrize("vec", [True, False])
def test_elementwise_kernels_past_the_grid_cap(dev, vec):
    """One count past the 8192-block cap per kernel and path: the grid-stride loops take a second trip.  Each element encodes its
    own index (i % 251 - 125), so a dropped, doubled or displaced element shows."""
    count = G.CAP_COUNT_VEC if vec else G.CAP_COUNT_SCALAR
    off = 0 if vec else 4
    assert G.ew_grid(count, vec) == (G.EW_GRID_CAP, 2)
    q = G.index_coded(count)
    scale = 2.0 ** -4
    x = G.calib_f32(q, scale)
    what = "past the grid cap, %s path" % ("vector" if vec else "scalar")
    assert G.calib_f2i_vec(off, 0) == vec and G.calib_i2f_vec(0, off) == vec and G.add_vec(off, 0, 0) == vec
    _same_i8(_calib_f2i(dev, x, scale, off, 0, what), q, "calib f32->i8 " + what)
    _same_bits(_calib_i2f(dev, q, scale, 0, off, what), x, "calib i8->f32 " + what)
    y = (np.arange(count, dtype=np.int64) % 241 * 256).astype(F32)
    for relu in (False, True):
        _same_bits(_add(dev, x, y, relu, off, 0, 0, what), G.add_ref(x, y, relu), "add relu %d " % relu + what)


# ------------------------------------------------------------------ 2. pool2d
def _pool(dev, x, typ, k, s, pads, exclusive=True, ceil_mode=False, what=""):
    ctx = dev.ctx
    i8 = x.dtype == np.int8
    n, c, h, w = x.shape
    d = importlib.import_module(type(ctx).__module__).PoolDesc()
    d.planes, d.h, d.w = n * c, h, w
    d.oh, d.ow = G.pool_out_hw(h, w, k, s, pads, ceil_mode)
    d.kh, d.kw = k, k
    d.pad[:] = list(pads)
    d.stride[:] = [s, s]
    d.is_max, d.exclusive = int(typ == "max"), int(exclusive)
    px = dev.put(x)
    py, fetch = dev.out((n, c, d.oh, d.ow), np.int8 if i8 else F32)
    fn = ctx.L.plhip_pool2d_max_i8 if i8 else ctx.L.plhip_pool2d_f32
    ctx.check(fn(ctx.h, C.byref(d), px, py), "pool2d")
    got = fetch(what)
    dev.release()
    return got


@pytest.fixture(scope="module")
def plane_sweep_refs(plref):
    """Inputs and oracle outputs at the largest plane count, once: planes are independent, so a smaller count is a prefix."""
    refs = {}
    pmax = max(G.PLANE_COUNTS)
    for (h, w, k, s, pads) in G.PLANE_SWEEP_GEOMS:
        xf, xi = G.pool_planes_f32(pmax, h, w), G.pool_planes_i8(pmax, h, w)
        r = {"xf": xf, "xi": xi, "i8": G.pool_i8_ref(plref, xi, k, s, pads)}
        for typ, excl in G.POOL_KINDS:
            r[(typ, excl)] = plref.pool2d(xf, typ, (k, k), (s, s), pads, exclusive=excl)
        refs[(h, w, k, s, pads)] = r
    return refs


@pytest.mark.parametrize("planes", G.PLANE_COUNTS)
def test_pool2d_plane_split_over_grid_z(dev, pkg, plane_sweep_refs, planes):
    """planes around and past 32768: plane = blockIdx.z * gridDim.y + blockIdx.y in all three pool kernels (the 5x9 k3 s2 p1
    geometry takes the int8 3x3 stride-2 kernel).  Every plane's values name the plane.  Bit for bit against the oracle."""
    assert G.pool_plane_split(planes) == (min(planes, G.POOL_GY), 1 if planes <= G.POOL_GY else 2 if planes <= 2 * G.POOL_GY else 3)
    routes = set()
    for geom, r in plane_sweep_refs.items():
        h, w, k, s, pads = geom
        for typ, excl in G.POOL_KINDS:
            what = "pool %s excl %d planes %d %r" % (typ, excl, planes, geom)
            _same_bits(_pool(dev, r["xf"][:, :planes], typ, k, s, pads, excl, what=what), r[(typ, excl)][:, :planes], what)
        what = "int8 max pool planes %d %r" % (planes, geom)
        _same_i8(_pool(dev, r["xi"][:, :planes], "max", k, s, pads, what=what), r["i8"][:, :planes], what)
        routes.add(G.pool_route(h, w, k, s, pads))
    assert routes == {"pool3x3s2_max_i8", "pool2d_max_i8"}


@pytest.mark.parametrize("ceil_mode", [False, True])
@pytest.mark.parametrize("geom", G.PAD_ONLY_GEOMS)
def test_pool2d_windows_that_cover_only_padding(dev, pkg, plref, geom, ceil_mode):
    """Windows wholly inside the bottom / right padding: 0 in those outputs, as pooling_basic and the oracle have it, from the
    fp32 kernel (max, both avg kinds) and from both int8 kernels."""
    h, w, k, s, pads = geom
    empty = G.pool_empty_windows(h, w, k, s, pads, ceil_mode)
    assert empty.any()
    rng = np.random.default_rng(700 + h * w)
    x = (rng.standard_normal((2, 3, h, w)) + 3).astype(F32)
    for typ, excl in G.POOL_KINDS:
        what = "pool %s excl %d %r ceil %d" % (typ, excl, geom, ceil_mode)
        want = plref.pool2d(x, typ, (k, k), (s, s), pads, exclusive=excl, ceil_mode=ceil_mode)
        got = _pool(dev, x, typ, k, s, pads, excl, ceil_mode, what)
        assert (got[:, :, empty] == 0).all(), what + ": a padding-only window is not 0"
        _same_bits(got, want, what)
    for kind in G.I8_VALUE_KINDS:
        what = "int8 max pool (%s, %s values) %r ceil %d" % (G.pool_route(h, w, k, s, pads, ceil_mode), kind, geom, ceil_mode)
        xi = G.pool_i8_values(kind, (2, 3, h, w), h + w)
        got = _pool(dev, xi, "max", k, s, pads, ceil_mode=ceil_mode, what=what)
        assert (got[:, :, empty] == 0).all(), what + ": a padding-only window is not 0: %r" % (got[0, 0].tolist(),)
        _same_i8(got, G.pool_i8_ref(plref, xi, k, s, pads, ceil_mode), what)


def test_pool2d_max_i8_both_kernels_at_value_edges(dev, pkg, plref):
    """Both int8 kernels (the host restatement of the launcher's choice says which case reaches which) on planes of all -128,
    planes whose only value above -128 sits in the last column or row, and values in -128..-101."""
    routes = {}
    for geom in G.I8_EXTRA_GEOMS + G.PAD_ONLY_GEOMS:
        h, w, k, s, pads = geom
        route = G.pool_route(h, w, k, s, pads)
        routes.setdefault(route, []).append(geom)
        if h * w > 1000:
            continue  # (ResNet50's pool1: the route only; test_int8_max_pool_commutes_with_calib runs it)
        for kind in G.I8_VALUE_KINDS:
            what = "int8 max pool (%s, %s values) %r" % (route, kind, geom)
            xi = G.pool_i8_values(kind, (2, 3, h, w), h * 31 + w)
            _same_i8(_pool(dev, xi, "max", k, s, pads, what=what), G.pool_i8_ref(plref, xi, k, s, pads), what)
    assert len(routes["pool3x3s2_max_i8"]) >= 4 and len(routes["pool2d_max_i8"]) >= 4
    assert (112, 112, 3, 2, (1, 1, 1, 1)) in routes["pool3x3s2_max_i8"]
    assert sum(g in routes["pool3x3s2_max_i8"] for g in G.PAD_ONLY_GEOMS) == 2 and G.PAD_ONLY_GEOMS[2] in routes["pool2d_max_i8"]


# ------------------------------------------------------------------ 3. global_avg_pool
def _gap(dev, x, what):
    ctx = dev.ctx
    nc, sp = x.shape
    px = dev.put(x)
    py, fetch = dev.out((nc,), F32)
    ctx.check(ctx.L.plhip_global_avg_pool_f32(ctx.h, px, nc, sp, py), "global_avg_pool")
    got = fetch(what)
    dev.release()
    return got


@pytest.mark.parametrize("spatial", G.GAP_SPATIAL)
def test_global_avg_pool_exact_on_integers_and_within_the_derived_bound(dev, spatial):
    """Integer-valued planes (|x| <= 64: every partial sum is an integer below 2^24, exact in any order, and the division is
    correctly rounded): the result is float32(float64 mean) bit for bit; each plane carries its own constant, so a plane in the
    wrong slot fails.

    Real-valued planes, N(0, 1) and 1000 + N(0, 1), against the float64 mean within a bound derived from the kernel's summation
    shape, not measured: a lane adds its ceil(spatial / 16) elements in order (the first add, to 0, is exact), the 16 lanes of
    a plane meet in four shuffle levels, and one division follows.  An element therefore passes through at most
    (ceil(spatial / 16) - 1) + 4 + 1 roundings, each (1 + d) with |d| <= 2^-24, so the computed mean is sum(x_i (1 + t_i)) /
    spatial with |t_i| <= gamma_k, k = ceil(spatial / 16) + 5 (one to spare), gamma_k = k 2^-24 / (1 - k 2^-24), and
    |err| <= gamma_k * mean|x|."""
    for nc in G.GAP_NC:
        x = G.gap_input("int", nc, spatial)
        what = "global_avg_pool integers nc %d spatial %d" % (nc, spatial)
        _same_bits(_gap(dev, x, what), G.gap_ref64(x).astype(F32), what)
        for kind in ("normal", "offset"):
            x = G.gap_input(kind, nc, spatial)
            what = "global_avg_pool %s nc %d spatial %d" % (kind, nc, spatial)
            err = np.abs(_gap(dev, x, what).astype(np.float64) - G.gap_ref64(x))
            bound = G.gap_bound(x)
            worst = int(np.argmax(err - bound))
            print("%s: max err %.3e, bound there %.3e" % (what, err[worst], bound[worst]))
            assert (err <= bound).all(), "%s: plane %d err %.3e > bound %.3e" % (what, worst, err[worst], bound[worst])


# ------------------------------------------------------------------ 4. softmax
def _softmax(dev, x, what):
    ctx = dev.ctx
    rows, cols = x.shape
    px = dev.put(x)
    py, fetch = dev.out(x.shape, F32)
    ctx.check(ctx.L.plhip_softmax_f32(ctx.h, px, rows, cols, py), "softmax")
    got = fetch(what)
    dev.release()
    return got


@pytest.mark.parametrize("cols", G.SOFTMAX_COLS)
def test_softmax_reductions_cannot_hide(dev, cols):
    """Against a float64 softmax at rtol 1e-5, atol 1e-7, on inputs where a wrong reduction shows:
    a dominant logit (+100 among -100) at the first and last position of waves and trips -- a maximum that misses it overflows
    expf; a uniform row -- every output is fl32(1 / cols) bit for bit (the sum of ones is exact, the division correctly
    rounded), a sum that misses a wave or a trip is off by a factor; N(0, 3) logits with a common offset of 0, +1e4, -1e4.

    Property on every random row: outputs in [0, 1] and their float64 sum within gamma_k + 2^-24 of 1.  The kernel computes
    e_i = expf(x_i - max) twice with the same result, s = the fp32 sum of the e_i and y_i = e_i / s.  A thread adds its
    ceil(cols / 256) values in order (the first add is exact), six shuffle levels make the wave's sum, two more adds join the
    four waves: each e_i reaches s through at most ceil(cols / 256) + 7 roundings, the division is one more, and all e_i are
    >= 0, so sum(y_i) = sum(e_i (1 + a_i)) / sum(e_i (1 + b_i)) lies within gamma_k of 1 for k = ceil(cols / 256) + 10 (two to
    spare); 2^-24 covers outputs that underflow."""
    x, ps = G.softmax_dominant(cols)
    got = _softmax(dev, x, "softmax dominant cols %d" % cols)
    want = np.zeros_like(x)
    want[np.arange(len(ps)), ps] = 1
    _same_bits(got, want, "softmax dominant logit, cols %d, positions %r" % (cols, ps))
    for rows in G.SOFTMAX_ROWS:
        what = "softmax uniform rows %d cols %d" % (rows, cols)
        got = _softmax(dev, G.softmax_uniform(rows, cols), what)
        _same_bits(got, np.full((rows, cols), F32(1) / F32(cols), F32), what)
        for offset in (0.0, 1e4, -1e4):
            x = G.softmax_random(rows, cols, offset)
            what = "softmax rows %d cols %d offset %g" % (rows, cols, offset)
            got = _softmax(dev, x, what)
            np.testing.assert_allclose(got, G.softmax_ref64(x), rtol=1e-5, atol=1e-7, err_msg=what)
            assert (got >= 0).all() and (got <= 1).all(), what
            dev_sum = np.abs(got.astype(np.float64).sum(axis=1) - 1)
            assert (dev_sum <= G.softmax_sum_bound(cols)).all(), "%s: row sums off by %.3e > %.3e" % (what, dev_sum.max(), G.softmax_sum_bound(cols))
    if cols == 1:
        assert (_softmax(dev, np.array([[3.5], [-1e30], [0.0]], F32), "cols 1") == 1).all()


# ------------------------------------------------------------------ 5. fc dispatch edges
def _fc(dev, packed, x, x_off, scale, bias, flags, out_kind, n, what):
    ctx = dev.ctx
    m, k = x.shape
    px = dev.put(x, x_off)
    ps = dev.put(scale) if scale is not None else C.c_void_p()
    pb = dev.put(bias) if bias is not None else C.c_void_p()
    dt = {0: np.int32, 1: F32, 2: np.int8}[out_kind]
    py, fetch = dev.out((m, n), dt)
    ctx.check(ctx.L.plhip_fc_int8(ctx.h, m, k, n, px, packed, ps, pb, int(flags), py, out_kind), "fc")
    got = fetch(what)
    dev.release()
    return got


def test_fc_dispatch_reaches_all_three_kernels(dev, pkg, plref):
    """launch_fc's choice by k % 16, k % 32, the alignment of x and the 64 KiB LDS bound, with no knob set: the fast kernel at
    exactly 64 KiB of dynamic LDS, the generic and the MFMA kernel past the bound, and a misaligned x on the generic and the
    MFMA kernel.  int32 accumulators, int8 and fp32 outputs (both rounding routes) bit for bit against the oracle."""
    capi, ctx = pkg.capi, dev.ctx
    assert not capi.KNOBS_SET.get("FC_MFMA")
    routes = [G.fc_route(k, off) for (_m, k, _n, off) in G.FC_CASES]
    assert routes == ["fc_fast", "fc_dot4", "fc_mfma", "fc_fast", "fc_dot4", "fc_mfma"]
    assert G.fc_lds_bytes(4096) == G.FC_LDS_BOUND
    for i, (m, k, n, off) in enumerate(G.FC_CASES):
        x, w, sc, sc8, bias = G.fc_inputs(m, k, n, k + n)
        with ctx.scope() as s:
            packed = s.alloc(ctx.L.plhip_fc_packed_weight_bytes(k, n))
            ctx.check(ctx.L.plhip_pack_fc_weights(ctx.h, k, n, s.put(w), packed), "pack_fc")
            what = "fc %s m %d k %d n %d x+%d" % (routes[i], m, k, n, off)
            y8, acc = plref.fc(x, w, bias, sc8, True, True)
            assert np.array_equal(_fc(dev, packed, x, off, None, None, 0, capi.OUT_I32, n, what), acc), what + ": int32 accumulators differ"
            _same_i8(_fc(dev, packed, x, off, sc8, bias, 1, capi.OUT_I8, n, what), y8, what + " int8 out")
            for relu in (0, 1):
                for route in (0, 1):
                    yf, _ = plref.fc(x, w, bias, sc, relu, False, route=route)
                    got = _fc(dev, packed, x, off, sc, bias, relu | (2 * route), capi.OUT_F32, n, what)
                    _same_bits(got, yf, what + " fp32 out relu %d route %d" % (relu, route))
            # no bias
            yf, _ = plref.fc(x, w, None, sc, 0, False, route=0)
            _same_bits(_fc(dev, packed, x, off, sc, None, 0, capi.OUT_F32, n, what), yf, what + " fp32 out, no bias")
