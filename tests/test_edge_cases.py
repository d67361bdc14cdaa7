"""CPU guard for the operands of test_gpu_edges.py: run through the oracle alone, every route's cases really reach the edges
the GPU test is there to pin (exact ties of each sign, +-127.5, both saturation bounds, the relu6 clip, fractions where a
round-to-nearest-even truncation differs from round-toward-zero, |acc| > 2^24).  Runs without a GPU."""
import numpy as np

import edge_cases as E


def _check(name, act, alpha, st):
    what = "%s act %d alpha %g: %s" % (name, act, alpha, st)
    n = st["n"]
    assert st["tie_pos"] >= 0.01 * n, what
    if act in (E.ACT_NONE, E.ACT_LEAKY):
        assert st["tie_neg"] >= 0.01 * n, what
        assert st["sat_neg"] > 0, what
    if act == E.ACT_NONE:
        assert st["at_m127_5"] > 0, what
    if not (act == E.ACT_RELU6 and alpha < 127):
        assert st["sat_pos"] > 0 and st["at_127_5"] > 0, what
    else:
        assert st["clip"] > 0, what
    assert st["rtz"] > 0, what


def test_generator_reaches_every_edge(plref):
    big = {}
    for i, route in enumerate(E.ROUTES):
        for j, (act, alpha) in enumerate(E.acts_of(route)):
            c = E.make_case(plref, route, act, alpha, False, E.case_seed(i, route, j))
            _check(route["name"], act, alpha, E.edge_stats(c["pre"], act, alpha))
            if route["kind"] in ("dwpw", "dwconv"):  # the depthwise stage of a fused pair sits on its edges too
                _check(route["name"] + " dw stage", c["dw_act"], c["dw_alpha"],
                       E.edge_stats(c["pre_mid"], c["dw_act"], c["dw_alpha"]))
            if route["kind"] == "tail":  # y + res on the calib's ties (2 z = k + 0.5), both signs
                st = E.edge_stats(c["pre_q"], E.ACT_NONE, 0.0)
                assert st["tie_pos"] > 0.01 * st["n"] and (st["tie_neg"] > 0.01 * st["n"] or act == E.ACT_RELU), st
            if route["kind"] == "fc":  # dyadic scales: the reference's one- and two-rounding fc forms agree bit for bit
                assert np.array_equal(c["ref_f32"].view(np.uint32), c["ref_f32_two_roundings"].view(np.uint32))
        c = E.make_case(plref, route, E.ACT_NONE, 0.0, True, E.case_seed(i, route, 0, True))
        big[route["name"]] = int(np.abs(c["acc"].astype(np.int64)).max())
        assert c["x"].min() == -128 or route["kind"] in ("calib", "image"), route["name"]
    over = {k for k, v in big.items() if v > 1 << 24}
    # every route whose K admits it (K > 1040: 1x1 GEMMs outside the K <= 1024 wide / areg forms, implicit GEMM, patch, im2col, fc)
    assert over == {r["name"] for r in E.ROUTES if r["mm_cin"] and r["mm_cin"] * r["shape"][5] * r["shape"][6] > 1040}, big
    assert len(over) >= 8, big


def test_every_route_reaches_the_kernel_it_names(pkg):
    """The route table against the library's own launch plan for the GEMM, depthwise and fused depthwise routes
    (edge_cases.kernel_of): each forced knob lands on its kernel -- for the direct depthwise kernel on the very instance (KS, S,
    RS, STAGE, FASTV) its row states -- for every output kind and for the maximum-magnitude K as well, and every kernel of the
    table is reached."""
    seen = set()
    for r in E.ROUTES:
        with E.Knobs(pkg.capi.load(), r["knobs"]):
            for cin in {r["shape"][1], r["mm_cin"] or r["shape"][1]}:
                for out in ("i32", "i8", "f32"):
                    k = E.kernel_of(pkg.capi, r, cin, out)
                    assert k == E.kernel_for(r, out), (r["name"], cin, out, k)
                    seen.add(k)
    assert {"gemm_nchw", "gemm_vperm_lds", "gemm_ring", "gemm_ring_ma1", "gemm_areg", "gemm_wide_n4", "gemm_wide_n7",
            "gemm_wide_n8", "dwpw_14x14", "dwpw_14x14_mtw2", "dwpw_stream", "dwpw_7x7", "dw_band", "dw_generic", "dw_conv1x1", "fc_dot4",
            "fc_mfma"} <= seen
    # the three strip heights, staged and not, the general row fetch, the 5x5 filter, stride 2
    assert {r["kernel"] for r in E.ROUTES if r["kernel"].startswith("dw_direct")} | {"dw_direct KS=3 S=1 RS=7 STAGE=0 FASTV=1"} <= seen
    for token in ("RS=4", "RS=7", "RS=8", "STAGE=0", "STAGE=1", "FASTV=0", "KS=5", "S=2"):
        assert any(token in k.split(" ") for k in seen), token
