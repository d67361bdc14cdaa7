"""Case generators and plain numpy / float64 references for the glue kernels (calib both ways, elementwise_add, pool2d,
global_avg_pool, softmax, the fc launcher's dispatch) at their alignment, grid and value edges.  TEST INFRASTRUCTURE, next to
edge_cases.py: nothing here touches the device side, so test_glue_cases.py checks every generator and reference on a CPU and
test_gpu_glue_edges.py runs the same cases through the C ABI.

The host restatements of launcher logic (pool_route, fc_route, ew_grid) follow paddle-lite_amd/csrc/eltwise_pool.hip and
misc_ops.hip line for line, as edge_cases.kernel_of does for the conv routes: a test asserts with them that its case list
reaches every kernel, the device run then shows that each kernel computes the same values."""
import functools
import math

import numpy as np

F32 = np.float32
FLT_MAX = F32(3.4028234663852886e38)
U = 2.0 ** -24  # unit roundoff of fp32


def gamma(k):
    """Higham's gamma_k for fp32: the relative error bound of k chained roundings."""
    return k * U / (1 - k * U)


# ------------------------------------------------------------------ calib and elementwise_add
COUNTS = (1, 3, 4, 5, 1023, 1024, 1025)
EW_GRID_CAP, EW_BLOCK = 8192, 256
CAP_COUNT_VEC = EW_GRID_CAP * EW_BLOCK * 4 + 5  # one element more than a full first trip of the vector loop, plus a scalar tail
CAP_COUNT_SCALAR = EW_GRID_CAP * EW_BLOCK + 3   # the same for the scalar loop
CALIB_SCALES = (2.0 ** -4, 1.0 / 31, 12.0 / 127)  # the first: inv = fl32(1 / scale) is exact, so (k + .5) * scale is a true tie


def ew_grid(count, vec):
    """(blocks, trips): ew_blocks / launch_eltwise_add's grid for `count` elements and the grid-stride trips of its main loop."""
    items = count >> 2 if vec else count
    blocks = min(max((items + EW_BLOCK - 1) // EW_BLOCK, 1), EW_GRID_CAP)
    return blocks, -(-items // (blocks * EW_BLOCK))


def calib_f2i_vec(x_off_bytes, y_off_bytes):
    """launch_calib_f32_to_i8's vector condition for bases that many bytes past a 16-byte boundary."""
    return x_off_bytes % 16 == 0 and y_off_bytes % 4 == 0


def calib_i2f_vec(x_off_bytes, y_off_bytes):
    return y_off_bytes % 16 == 0 and x_off_bytes % 4 == 0


def add_vec(*off_bytes):
    return all(o % 16 == 0 for o in off_bytes)


def calib_i8(x, scale):
    """calib[fp32_to_int8]: round half away from zero of fl32(x * fl32(1 / scale)), clamped to +-127 (mbv3_oracle.calib_i8 says
    the same in other words; test_glue_cases.py holds the two and the C oracle together)."""
    inv = F32(1.0) / F32(scale)
    with np.errstate(all="ignore"):
        v = (np.asarray(x, F32) * inv).astype(F32).astype(np.float64)
    r = np.sign(v) * np.floor(np.abs(v) + 0.5)
    return np.clip(r, -127, 127).astype(np.int8)


def calib_f32(q, scale):
    """calib[int8_to_fp32]: one fp32 multiply."""
    return (np.asarray(q, np.int8).astype(F32) * F32(scale)).astype(F32)


def add_ref(x, y, relu):
    """x + y in fp32, then r > 0 ? r : 0 (so relu(-0.0) is +0.0)."""
    with np.errstate(all="ignore"):
        r = (np.asarray(x, F32) + np.asarray(y, F32)).astype(F32)
    return np.where(r > 0, r, F32(0)).astype(F32) if relu else r


def calib_tie_values(scale):
    """x = (k + 0.5) * scale, k = -128..127: with a power-of-two scale every one is an exact tie of x * inv."""
    return ((np.arange(-128, 128) + 0.5) * scale).astype(F32)


def calib_edge_values(scale):
    """Ties of both signs, +-126.5 / +-127.5 (the last value below and the first at the bound), past both bounds, +-inf, +-0
    and near-ties one fp32 step to either side.  No NaN, no denormals: the reference does not define them."""
    s = float(scale)
    t = calib_tie_values(scale)
    e = np.array([126.5 * s, -126.5 * s, 127.5 * s, -127.5 * s, 127.49 * s, -127.49 * s, 128 * s, -128 * s, 200 * s, -200 * s,
                  1e30, -1e30, np.inf, -np.inf, 0.0, -0.0, 0.49 * s, -0.49 * s], F32)
    return np.concatenate([e, t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf))]).astype(F32)


def calib_f2i_input(scale, count, seed):
    """`count` values: the edge values rotated by the seed (so that even count 1 meets several of them over the sweep), then
    values spread over +-140 steps of the scale."""
    e = np.roll(calib_edge_values(scale), -7 * seed)
    rng = np.random.default_rng(1000 + seed)
    x = (rng.uniform(-140, 140, count) * scale).astype(F32)
    k = min(count, e.size)
    x[:k] = e[:k]
    return x


def calib_i2f_input(count, seed):
    """Every int8 value, -128 included, in a rotating order."""
    return ((np.arange(count) * 37 + 11 * seed) % 256 - 128).astype(np.int8)


def add_edge_pairs():
    """+-0 in every pairing, FLT_MAX + FLT_MAX, inf plus finite, exact cancellation, a sum that rounds.  No NaN (so no
    inf - inf)."""
    z = [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)]
    o = [(FLT_MAX, FLT_MAX), (-FLT_MAX, -FLT_MAX), (np.inf, 1.0), (-np.inf, 1.0), (1.0, np.inf), (np.inf, np.inf), (-np.inf, -np.inf),
         (np.inf, -FLT_MAX), (1.5, -1.5), (-3e38, 3e38), (1e-30, -1e-30), (1.0, 2.0 ** -24), (1.0, -2.0 ** -25), (16777216.0, 1.0),
         (-2.5, 1.0), (1e-38, -2e-38)]
    p = np.array(z + o, F32)
    return p[:, 0].copy(), p[:, 1].copy()


def add_input(count, seed):
    ex, ey = add_edge_pairs()
    ex, ey = np.roll(ex, -5 * seed), np.roll(ey, -5 * seed)
    rng = np.random.default_rng(2000 + seed)
    x, y = rng.standard_normal(count).astype(F32), rng.standard_normal(count).astype(F32)
    k = min(count, ex.size)
    x[:k], y[:k] = ex[:k], ey[:k]
    return x, y


def index_coded(count):
    """q[i] = i % 251 - 125 as int8: 251 is prime to every power of two, so a dropped, doubled or displaced element of a
    grid-stride loop changes the sequence."""
    return (np.arange(count, dtype=np.int64) % 251 - 125).astype(np.int8)


# ------------------------------------------------------------------ pool2d
POOL_GY = 32768  # launch_pool2d*: gridDim.y = min(planes, 32768), the rest of the planes go to gridDim.z
PLANE_COUNTS = (32767, 32768, 32769, 65536, 65539)
# (h, w, k, s, pads {top, bottom, left, right}): tiny planes; the second takes the int8 3x3 stride-2 kernel
PLANE_SWEEP_GEOMS = ((4, 4, 2, 2, (0, 0, 0, 0)), (5, 9, 3, 2, (1, 1, 1, 1)))
# windows that cover padding only (bottom rows of the first, right columns of the second, both of the third)
PAD_ONLY_GEOMS = ((4, 8, 3, 2, (0, 3, 1, 1)), (5, 10, 3, 2, (1, 1, 0, 4)), (4, 6, 2, 2, (0, 2, 0, 2)))
POOL_KINDS = (("max", True), ("avg", True), ("avg", False))  # (pooling_type, exclusive) of the fp32 kernel
# further int8 geometries on both sides of the fast kernel's condition
I8_EXTRA_GEOMS = ((5, 9, 3, 2, (1, 1, 1, 1)), (13, 17, 3, 2, (0, 1, 1, 2)), (3, 4, 3, 2, (1, 1, 1, 1)), (112, 112, 3, 2, (1, 1, 1, 1)),
                  (7, 9, 2, 2, (0, 0, 0, 0)), (6, 6, 3, 3, (1, 1, 1, 1)), (9, 9, 3, 2, (2, 2, 2, 2)), (3, 3, 3, 2, (1, 1, 1, 1)),
                  (9, 12, 3, 2, (1, 1, 2, 1)))
I8_VALUE_KINDS = ("random", "all_m128", "last_col", "last_row", "low")


def pool_out_size(i, k, p0, p1, s, ceil_mode):
    """PoolOutputSize (pool_op.cc:44-61)."""
    return (i - k + p0 + p1 + (s - 1 if ceil_mode else 0)) // s + 1


def pool_out_hw(h, w, k, s, pads, ceil_mode):
    return pool_out_size(h, k, pads[0], pads[1], s, ceil_mode), pool_out_size(w, k, pads[2], pads[3], s, ceil_mode)


def pool_geometry_ok(h, w, oh, ow, k, s, pads):
    """pool2d_impl's descriptor check: every window starts inside the padded image."""
    if min(h, w, oh, ow, k, s) < 1 or min(pads) < 0:
        return False
    return not ((oh - 1) * s - pads[0] >= h + pads[1] or (ow - 1) * s - pads[2] >= w + pads[3])


def pool_empty_windows(h, w, k, s, pads, ceil_mode):
    """bool [oh, ow]: the outputs whose window, clipped to the image, holds no element."""
    oh, ow = pool_out_hw(h, w, k, s, pads, ceil_mode)
    ys, xs = np.arange(oh) * s - pads[0], np.arange(ow) * s - pads[2]
    er = np.minimum(ys + k, h) <= np.maximum(ys, 0)
    ec = np.minimum(xs + k, w) <= np.maximum(xs, 0)
    return er[:, None] | ec[None, :]


def pool_route(h, w, k, s, pads, ceil_mode=False):
    """launch_pool2d_max_i8's choice: "pool3x3s2_max_i8" (12-byte row windows) or "pool2d_max_i8" (the generic kernel)."""
    _oh, ow = pool_out_hw(h, w, k, s, pads, ceil_mode)
    owq = (ow + 3) >> 2
    fast = k == 3 and s == 2 and pads[0] <= 1 and pads[2] <= 1 and w >= 4 and h * w >= 12 and 8 * (owq - 1) - pads[2] < w
    return "pool3x3s2_max_i8" if fast else "pool2d_max_i8"


def pool_plane_split(planes):
    """(gridDim.y, gridDim.z) of the pool launches."""
    gy = min(planes, POOL_GY)
    return gy, (planes + gy - 1) // gy


def pool_planes_f32(planes, h, w):
    """[1, planes, h, w] fp32: plane p holds p plus a permutation of (0 .. h*w-1) / 64 that depends on p, so every value names
    its plane, is exact in fp32, and no two elements of a plane are equal."""
    p = np.arange(planes, dtype=np.int64)[:, None]
    i = np.arange(h * w, dtype=np.int64)[None, :]
    step = 7 if (h * w) % 7 else 11
    frac = (i * step + p) % (h * w)
    return (p + frac / 64.0).astype(F32).reshape(1, planes, h, w)


def pool_planes_i8(planes, h, w):
    """[1, planes, h, w] int8: a pattern that differs between neighbouring planes and between planes 32768 apart."""
    p = np.arange(planes, dtype=np.int64)[:, None]
    i = np.arange(h * w, dtype=np.int64)[None, :]
    return ((p * 37 + (p >> 8) * 3 + i * 11) % 255 - 127).astype(np.int8).reshape(1, planes, h, w)


def pool_i8_values(kind, shape, seed):
    """int8 planes [n, c, h, w]: "random" -127..127 with some -128; "all_m128"; "last_col" / "last_row": -128 everywhere but
    one value in the last column / row of each plane; "low": -128..-101, where a padding byte of 0 or -128 would win or lose."""
    rng = np.random.default_rng(3000 + seed)
    n, c, h, w = shape
    if kind == "random":
        x = rng.integers(-128, 128, shape).astype(np.int8)
    elif kind == "low":
        x = rng.integers(-128, -100, shape).astype(np.int8)
    else:
        x = np.full(shape, -128, np.int8)
        if kind == "last_col":
            x[:, :, rng.integers(0, h), w - 1] = -77
        elif kind == "last_row":
            x[:, :, h - 1, rng.integers(0, w)] = 5
        else:
            assert kind == "all_m128"
    return x


def pool_i8_ref(plref, x, k, s, pads, ceil_mode=False):
    """The oracle's fp32 max pool on the int8 values (exact), back to int8: 0 where a window is empty."""
    return plref.pool2d(x.astype(F32), "max", (k, k), (s, s), pads, ceil_mode=ceil_mode).astype(np.int8)


# ------------------------------------------------------------------ global_avg_pool
GAP_SPATIAL = (1, 2, 15, 16, 17, 49, 196, 3136, 12544)
GAP_NC = (1, 15, 16, 17, 33, 2 * 960)
GAP_LANES = 16  # lanes per plane in global_avg_pool_kernel


def gap_k(spatial):
    """Roundings on the path of one element: ceil(spatial / 16) sequential adds in its lane (the first, 0 + x, is exact), four
    shuffle levels, one division -- ceil(spatial / 16) + 5 bounds them with one to spare."""
    return -(-spatial // GAP_LANES) + 5


def gap_bound(x):
    """|kernel - float64 mean| <= gamma_k * mean|x| per plane; x [nc, spatial]."""
    return gamma(gap_k(x.shape[1])) * np.abs(x.astype(np.float64)).mean(axis=1)


@functools.lru_cache(maxsize=None)
def _normal_pool():
    n = max(GAP_SPATIAL) * max(GAP_NC)
    return np.random.default_rng(4000).standard_normal(n, dtype=F32)


def gap_input(kind, nc, spatial):
    """[nc, spatial] fp32.  "int": integers in -32..32 plus a per-plane constant in -32..32 (|x| <= 64: every partial sum is an
    integer below 2^24, exact in any order); "normal": N(0, 1); "offset": 1000 + N(0, 1)."""
    if kind == "int":
        rng = np.random.default_rng(4100 + 31 * nc + spatial % 1009)
        c = (np.arange(nc) * 7 % 65 - 32)[:, None]
        return (rng.integers(-32, 33, (nc, spatial)) + c).astype(F32)
    x = _normal_pool()[:nc * spatial].reshape(nc, spatial)
    return (x + F32(1000)).astype(F32) if kind == "offset" else x.copy()


def gap_ref64(x):
    return x.astype(np.float64).mean(axis=1)


def gap_emulate(x):
    """global_avg_pool_kernel's summation in numpy fp32: lane `sub` adds elements sub, sub + 16, ... in order, the 16 lanes
    meet in a butterfly (xor 8, 4, 2, 1), one division."""
    nc, sp = x.shape
    t = -(-sp // GAP_LANES)
    xp = np.zeros((nc, t * GAP_LANES), F32)  # (adding the zero padding is exact)
    xp[:, :sp] = x
    xp = xp.reshape(nc, t, GAP_LANES)
    s = np.zeros((nc, GAP_LANES), F32)
    for i in range(t):
        s = (s + xp[:, i]).astype(F32)
    for off in (8, 4, 2, 1):
        s = (s + s[:, np.arange(GAP_LANES) ^ off]).astype(F32)
    return (s[:, 0] / F32(sp)).astype(F32)


# ------------------------------------------------------------------ softmax
SOFTMAX_COLS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 1001, 4099)
SOFTMAX_ROWS = (1, 3, 128)
SOFTMAX_BLOCK = 256
DOMINANT_POS = (0, 63, 64, 128, 255, 256, -1)


def softmax_ref64(x):
    """float64 softmax of the fp32 logits."""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax_k(cols):
    """Roundings between an exp value and its output: ceil(cols / 256) sequential adds in its thread (the first is exact), six
    shuffle levels inside the wave, two adds across the four waves, one division: ceil(cols / 256) + 8; + 10 leaves two."""
    return -(-cols // SOFTMAX_BLOCK) + 10


def softmax_sum_bound(cols):
    """|float64 sum of a row's outputs - 1| <= gamma_k + 2^-24."""
    return gamma(softmax_k(cols)) + U


def softmax_dominant(cols):
    """One row per position p of DOMINANT_POS that exists: -100 everywhere, +100 at p.  Returns (x, positions)."""
    ps = sorted({p if p >= 0 else cols - 1 for p in DOMINANT_POS if p < cols})
    x = np.full((len(ps), cols), -100, F32)
    x[np.arange(len(ps)), ps] = 100
    return x, ps


def softmax_uniform(rows, cols):
    """Row r is the constant r / 2 - 3: every output is fl32(1 / cols)."""
    return np.repeat((np.arange(rows) * 0.5 - 3).astype(F32)[:, None], cols, axis=1)


def softmax_random(rows, cols, offset):
    """N(0, 3) logits plus a common offset (0, +1e4, -1e4), rounded to fp32."""
    rng = np.random.default_rng(5000 + 7 * rows + cols)
    return (offset + 3 * rng.standard_normal((rows, cols))).astype(F32)


def softmax_emulate(x):
    """softmax_kernel's reductions in numpy fp32 (numpy's exp in place of expf: the bound holds for any exp values, as long as
    both passes use the same ones).  Thread t takes columns t, t + 256, ...; shfl_down 32..1 leaves the wave's sum in lane 0;
    the four waves meet as (r0 + r1) + (r2 + r3)."""
    rows, cols = x.shape
    t = -(-cols // SOFTMAX_BLOCK)
    xp = np.full((rows, t * SOFTMAX_BLOCK), -np.inf, F32)
    xp[:, :cols] = x
    xp = xp.reshape(rows, t, SOFTMAX_BLOCK)
    mx = xp.max(axis=(1, 2), keepdims=True)
    with np.errstate(all="ignore"):
        e = np.exp((xp - mx).astype(F32)).astype(F32)  # exp(-inf) = 0 for the padding: adding it is exact
    s = np.zeros((rows, SOFTMAX_BLOCK), F32)
    for i in range(t):
        s = (s + e[:, i]).astype(F32)
    s = s.reshape(rows, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        sh = np.zeros_like(s)
        sh[:, :, :64 - off] = s[:, :, off:]  # (what lanes past the wave's end contribute never reaches lane 0)
        s = (s + sh).astype(F32)
    r = s[:, :, 0]
    tot = ((r[:, 0] + r[:, 1]).astype(F32) + (r[:, 2] + r[:, 3]).astype(F32)).astype(F32)
    y = (e.reshape(rows, -1)[:, :cols] / tot[:, None]).astype(F32)
    return y


# ------------------------------------------------------------------ fc dispatch
FCF_MB = 16
FC_LDS_BOUND = 64 * 1024
# (m, k, n, byte offset of x past a 16-byte boundary)
FC_CASES = ((17, 4096, 65, 0), (17, 4112, 65, 0), (17, 4128, 65, 0), (9, 48, 37, 0), (9, 48, 37, 1), (9, 64, 37, 1))


def fc_route(k, x_off_bytes, mfma_knob=0):
    """launch_fc's choice: "fc_fast" (x rows staged in LDS), "fc_mfma" or "fc_dot4" (the generic kernel)."""
    lds = max(FCF_MB * k, 4 * FCF_MB * 64 * 4)
    fast_ok = k % 16 == 0 and x_off_bytes % 16 == 0 and lds <= FC_LDS_BOUND
    if (mfma_knob or not fast_ok) and k % 32 == 0:
        return "fc_mfma"
    return "fc_fast" if fast_ok else "fc_dot4"


def fc_lds_bytes(k):
    return max(FCF_MB * k, 4 * FCF_MB * 64 * 4)


def fc_inputs(m, k, n, seed):
    """x [m, k], w [k, n] int8, the folded fp32-out and int8-out scales and a bias.  The last four k positions of every x row
    hold +-127 and -128 against nonzero weights: the bytewise tail quad and the last split-K slice carry weight."""
    rng = np.random.default_rng(6000 + seed)
    x = rng.integers(-127, 128, (m, k)).astype(np.int8)
    w = rng.integers(-127, 128, (k, n)).astype(np.int8)
    tail = np.array([127, -128, -127, 127, -128, -128, 127, -127], np.int8)
    for r in range(m):
        x[r, k - 4:] = np.roll(tail, r)[:4]
    w[k - 4:][w[k - 4:] == 0] = 3
    sc = ((1 + np.arange(n) % 5) * 1.7 / 127 / 127 / 3).astype(F32)
    sc8 = ((1 + np.arange(n) % 5) * 25.0 / (math.sqrt(k) * 73 * 73)).astype(F32)
    bias = rng.uniform(-1, 1, n).astype(F32)
    return x, w, sc, sc8, bias


# ------------------------------------------------------------------ se_gate
SE_EXTRA_PAIRS = ((10, 9), (13, 8), (959, 239), (960, 8), (8, 8), (261, 257))  # (C, Cr) outside both network tables
