"""CPU: the generators, numpy references and launcher restatements of glue_cases.py, held against the C oracle and against
their own claims (ties are ties, padding-only windows exist, every kernel is reached, the summation emulations stay inside the
derived bounds).  test_gpu_glue_edges.py runs the same cases on the device."""
import numpy as np
import pytest

import glue_cases as G
import mbv3_oracle as M

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_calib_references_equal_the_oracle_and_ties_are_ties(plref):
    for scale in G.CALIB_SCALES:
        x = np.concatenate([G.calib_edge_values(scale)] + [G.calib_f2i_input(scale, c, 3 * c) for c in G.COUNTS])
        q = G.calib_i8(x, scale)
        assert np.array_equal(q, plref.calib_f32_to_i8(x, scale)) and np.array_equal(q, M.calib_i8(x, scale))
        assert q.min() == -127 and q.max() == 127
        assert not np.isnan(x).any() and ((x == 0) | (np.abs(x) >= np.finfo(F32).tiny)).all()  # no NaN, no denormals
        qq = G.calib_i2f_input(1025, 5)
        assert set(qq.tolist()) == set(range(-128, 128))
        assert np.array_equal(_bits(G.calib_f32(qq, scale)), _bits(plref.calib_i8_to_f32(qq, scale)))
    # a power-of-two scale: inv is exact and every (k + .5) * scale is a tie, rounded away from zero
    scale = G.CALIB_SCALES[0]
    inv = F32(1) / F32(scale)
    assert float(inv) * scale == 1.0
    t = G.calib_tie_values(scale)
    prod = (t * inv).astype(F32).astype(np.float64)
    assert np.array_equal(prod, t.astype(np.float64) / scale)  # the product is exact
    assert (np.abs(prod - np.trunc(prod)) == 0.5).all() and (prod < 0).sum() == 128
    k = np.arange(-128, 128)
    assert np.array_equal(G.calib_i8(t, scale), np.clip(np.where(k >= 0, k + 1, k), -127, 127))
    e = G.calib_edge_values(scale)
    for v in (126.5, -126.5, 127.5, -127.5, np.inf, -np.inf):
        assert (e == F32(v * scale)).any()
    assert (_bits(e) == 0).any() and (_bits(e) == 0x80000000).any()
    # the other two scales: inv is inexact
    for scale in G.CALIB_SCALES[1:]:
        assert float(F32(1) / F32(scale)) * float(F32(scale)) != 1.0 or float(F32(scale)) != scale


def test_add_reference_equals_the_oracle(plref):
    ex, ey = G.add_edge_pairs()
    assert {(a, b) for a, b in zip(_bits(ex)[:4].tolist(), _bits(ey)[:4].tolist())} == {(0, 0), (0, 1 << 31), (1 << 31, 0), (1 << 31, 1 << 31)}
    for relu in (False, True):
        r = G.add_ref(ex, ey, relu)
        assert not np.isnan(r).any()
        assert np.array_equal(_bits(r), _bits(plref.elementwise_add(ex, ey, relu)))
        assert _bits(r)[3] == (0 if relu else 1 << 31) and _bits(r)[1] == 0  # relu(-0 + -0) is +0; +0 + -0 is +0
        assert np.isinf(r[4]) and (r == 0).sum() >= 6
        for c in G.COUNTS:
            x, y = G.add_input(c, c)
            assert np.array_equal(_bits(G.add_ref(x, y, relu)), _bits(plref.elementwise_add(x, y, relu)))


def test_grid_cap_counts_take_a_second_trip():
    assert G.ew_grid(G.CAP_COUNT_VEC, True) == (G.EW_GRID_CAP, 2) and G.ew_grid(G.CAP_COUNT_VEC - 5, True) == (G.EW_GRID_CAP, 1)
    assert G.ew_grid(G.CAP_COUNT_SCALAR, False) == (G.EW_GRID_CAP, 2) and G.ew_grid(G.CAP_COUNT_SCALAR - 3, False) == (G.EW_GRID_CAP, 1)
    assert G.CAP_COUNT_VEC % 4 == 1  # and a scalar tail after the vector loop
    assert max(G.ew_grid(c, v)[1] for c in G.COUNTS for v in (True, False)) == 1
    q = G.index_coded(2000)
    assert q.min() == -125 and q.max() == 125 and q[251] == q[0] and q[250] != q[0]
    assert G.calib_f2i_vec(0, 0) and not G.calib_f2i_vec(4, 0) and not G.calib_f2i_vec(0, 1) and G.calib_f2i_vec(0, 4)
    assert G.calib_i2f_vec(0, 0) and not G.calib_i2f_vec(1, 0) and not G.calib_i2f_vec(0, 4)
    assert G.add_vec(0, 0, 0) and not G.add_vec(0, 0, 4) and not G.add_vec(4, 0, 0)
    x = G.calib_f32(G.index_coded(5000), 2.0 ** -4)
    assert np.array_equal(G.calib_i8(x, 2.0 ** -4), G.index_coded(5000))


def test_pool_cases_and_routes(plref):
    # the padding-only cases: a window is empty with and without ceil_mode, the geometry passes the descriptor check, the
    # oracle writes 0 there
    for (h, w, k, s, pads) in G.PAD_ONLY_GEOMS:
        for ceil in (False, True):
            oh, ow = G.pool_out_hw(h, w, k, s, pads, ceil)
            assert oh == plref.lib().plref_pool_out_size(h, k, pads[0], pads[1], s, int(ceil))
            assert G.pool_geometry_ok(h, w, oh, ow, k, s, pads)
            empty = G.pool_empty_windows(h, w, k, s, pads, ceil)
            assert empty.shape == (oh, ow) and empty.any() and not empty.all()
            x = (np.random.default_rng(1).standard_normal((1, 2, h, w)) + 3).astype(F32)
            for typ, excl in G.POOL_KINDS:
                y = plref.pool2d(x, typ, (k, k), (s, s), pads, exclusive=excl, ceil_mode=ceil)
                assert (y[:, :, empty] == 0).all() and (y[:, :, ~empty] != 0).all(), (h, w, typ, excl, ceil)
            for kind in G.I8_VALUE_KINDS:
                xi = G.pool_i8_values(kind, (2, 3, h, w), 9)
                y = G.pool_i8_ref(plref, xi, k, s, pads, ceil)
                assert (y[:, :, empty] == 0).all() and (y[:, :, ~empty] != 0).all(), kind
                assert (y[:, :, ~empty] == -128).any() == (kind in ("all_m128", "last_col", "last_row")), kind
    assert not G.pool_geometry_ok(4, 4, 4, 2, 2, 2, (0, 0, 0, 0))
    assert G.pool_empty_windows(4, 8, 3, 2, (0, 3, 1, 1), False)[2].all() and G.pool_empty_windows(5, 10, 3, 2, (1, 1, 0, 4), False)[:, 5].all()
    # both int8 kernels over the case lists; the padding-only 3x3 stride-2 cases and ResNet50's pool1 on the fast side
    routes = {g: G.pool_route(*g) for g in G.I8_EXTRA_GEOMS + G.PAD_ONLY_GEOMS + G.PLANE_SWEEP_GEOMS}
    assert set(routes.values()) == {"pool3x3s2_max_i8", "pool2d_max_i8"}
    assert routes[(112, 112, 3, 2, (1, 1, 1, 1))] == "pool3x3s2_max_i8"
    assert [routes[g] for g in G.PAD_ONLY_GEOMS] == ["pool3x3s2_max_i8", "pool3x3s2_max_i8", "pool2d_max_i8"]
    assert [G.pool_route(*g, ceil_mode=True) for g in G.PAD_ONLY_GEOMS] == ["pool3x3s2_max_i8", "pool3x3s2_max_i8", "pool2d_max_i8"]
    assert [routes[g] for g in G.PLANE_SWEEP_GEOMS] == ["pool2d_max_i8", "pool3x3s2_max_i8"]
    assert G.pool_route(9, 9, 3, 2, (2, 2, 2, 2)) == "pool2d_max_i8" and G.pool_route(3, 3, 3, 2, (1, 1, 1, 1)) == "pool2d_max_i8"
    # the plane split: one z slice up to 32768 planes, then two, then three
    assert [G.pool_plane_split(p) for p in G.PLANE_COUNTS] == [(32767, 1), (32768, 1), (32768, 2), (32768, 2), (32768, 3)]
    for (h, w, k, s, pads) in G.PLANE_SWEEP_GEOMS:
        assert h * w <= 45
        xf, xi = G.pool_planes_f32(40000, h, w), G.pool_planes_i8(40000, h, w)
        assert np.array_equal(np.floor(xf[0]).reshape(40000, -1), np.repeat(np.arange(40000)[:, None], h * w, 1))
        assert all(np.unique(xf[0, p]).size == h * w for p in (0, 1, 32768, 39999))
        y = G.pool_i8_ref(plref, xi, k, s, pads)[0]
        assert not np.array_equal(y[:7232], y[32768:]) and (y[:-1] != y[1:]).any(axis=(1, 2)).all()


def test_global_avg_pool_references_and_bound(plref):
    for spatial in G.GAP_SPATIAL:
        for nc in (1, 17, 33):
            xi = G.gap_input("int", nc, spatial)
            assert np.abs(xi).max() <= 64 and np.array_equal(xi, np.round(xi))
            want = G.gap_ref64(xi).astype(F32)
            assert np.array_equal(_bits(want), _bits(plref.global_avg_pool(xi.reshape(1, nc, spatial, 1)).ravel()))
            assert np.array_equal(_bits(G.gap_emulate(xi)), _bits(want))  # exact whatever the order
            for kind in ("normal", "offset"):
                x = G.gap_input(kind, nc, spatial)
                ref = G.gap_ref64(x)
                np.testing.assert_allclose(plref.global_avg_pool(x.reshape(1, nc, spatial, 1)).ravel(), ref, rtol=2.0 ** -23)
                assert (np.abs(G.gap_emulate(x).astype(np.float64) - ref) <= G.gap_bound(x)).all(), (kind, nc, spatial)
    assert G.gap_k(1) == 6 and G.gap_k(16) == 6 and G.gap_k(17) == 7 and G.gap_k(12544) == 789
    x = G.gap_input("offset", 2 * 960, 3136)
    assert (np.abs(G.gap_emulate(x).astype(np.float64) - G.gap_ref64(x)) <= G.gap_bound(x)).all()
    assert abs(float(x.mean()) - 1000) < 1 and 0.5 < G.gap_bound(x)[0] / (G.gamma(201) * 1000) < 2
    xi = G.gap_input("int", 2 * 960, 49)
    assert np.unique(G.gap_ref64(xi)).size > 1000  # planes tell themselves apart


def test_softmax_references_and_bound(plref):
    for cols in G.SOFTMAX_COLS:
        x, ps = G.softmax_dominant(cols)
        assert ps == sorted(set(ps)) and ps[0] == 0 and ps[-1] == cols - 1 and all(p in ps for p in (63, 64, 128, 255, 256) if p < cols)
        want = np.zeros_like(x)
        want[np.arange(len(ps)), ps] = 1
        assert np.array_equal(G.softmax_ref64(x).astype(F32), want) and np.array_equal(plref.softmax(x), want)
        assert np.array_equal(G.softmax_emulate(x), want)
        u = G.softmax_uniform(3, cols)
        assert np.array_equal(_bits(G.softmax_emulate(u)), _bits(np.full((3, cols), F32(1) / F32(cols), F32)))
        np.testing.assert_allclose(G.softmax_ref64(u), 1.0 / cols, rtol=1e-12)
        for rows in (1, 3):
            for offset in (0.0, 1e4, -1e4):
                x = G.softmax_random(rows, cols, offset)
                assert abs(float(x.mean()) - offset) < 10
                ref = G.softmax_ref64(x)
                np.testing.assert_allclose(plref.softmax(x), ref, rtol=1e-5, atol=1e-7)
                y = G.softmax_emulate(x)
                np.testing.assert_allclose(y, ref, rtol=1e-5, atol=1e-7)
                assert (y >= 0).all() and (y <= 1).all()
                assert (np.abs(y.astype(np.float64).sum(axis=1) - 1) <= G.softmax_sum_bound(cols)).all(), (cols, offset)
    assert G.softmax_k(256) == 11 and G.softmax_k(257) == 12 and G.softmax_k(4099) == 27
    assert G.softmax_uniform(3, 5)[:, 0].tolist() == [-3.0, -2.5, -2.0]


def test_fc_cases_reach_all_three_kernels(plref):
    routes = [G.fc_route(k, off) for (_m, k, _n, off) in G.FC_CASES]
    assert routes == ["fc_fast", "fc_dot4", "fc_mfma", "fc_fast", "fc_dot4", "fc_mfma"]
    assert G.fc_lds_bytes(4096) == G.FC_LDS_BOUND and G.fc_lds_bytes(4112) > G.FC_LDS_BOUND and G.fc_lds_bytes(48) == 16384
    assert G.fc_route(1024, 0) == "fc_fast" and G.fc_route(1024, 0, mfma_knob=1) == "fc_mfma" and G.fc_route(67, 0) == "fc_dot4"
    for (m, k, n, off) in G.FC_CASES:
        x, w, sc, sc8, bias = G.fc_inputs(m, k, n, k + n)
        assert set(np.abs(x[:, k - 4:].astype(int)).ravel().tolist()) <= {127, 128} and (x[:, k - 4:] == -128).any() and (w[k - 4:] != 0).all()
        y8, acc = plref.fc(x, w, bias, sc8, True, True)
        assert np.array_equal(acc, x.astype(np.int64) @ w.astype(np.int64))
        assert y8.max() == 127 and ((y8 > 0) & (y8 < 127)).mean() > 0.2, (m, k, n)  # the int8 scale spreads the outputs
        y0, _ = plref.fc(x, w, bias, sc, 0, False, route=0)
        y1, _ = plref.fc(x, w, bias, sc, 0, False, route=1)
        np.testing.assert_allclose(y0, acc * sc.astype(np.float64) + bias, rtol=1e-6, atol=1e-6)
        assert (_bits(y0) != _bits(y1)).any()  # the two rounding routes differ on these inputs


def test_se_extra_pairs_lie_outside_the_network_tables(pkg=None):
    assert all(8 <= c <= 960 and 8 <= cr <= 960 for c, cr in G.SE_EXTRA_PAIRS)
    assert any(c % 4 and cr % 4 for c, cr in G.SE_EXTRA_PAIRS) and sum(bool(c % 4 or cr % 4) for c, cr in G.SE_EXTRA_PAIRS) >= 4
