"""CPU guard for test_gpu_dwconv_envelope.py: the case table of dwconv_cases.py against the library's own launch plan and
against the oracle alone.  Every case is one fusion G accepts, sits in the regime of dw_conv1x1_launch_plan it claims, the table
as a whole covers every regime, and the cases with stated seeds really put the depthwise stage, the 1x1 stage and the calib
copies on their value edges.  The binding's misalign / sentinel arguments are checked over test_capi_scope_host.py's stub
library.  Runs without a GPU."""
import ctypes

import numpy as np
import pytest

import dwconv_cases as D
import edge_cases as E
from test_capi_scope_host import stub_context


@pytest.fixture(scope="module")
def plans(pkg):
    """name -> the plan of the case under the alignment it runs with (fp32 output, no tail)."""
    return {c["name"]: D.plan_of(pkg.capi, c) for c in D.CASES}


def test_every_case_is_inside_the_envelope(pkg, plans):
    L = pkg.capi.load()
    assert len(D.BY_NAME) == len(D.CASES)
    for c in D.CASES:
        d = D.desc_of(pkg.capi, c["shape"])
        m = c["shape"][6]
        for out, tail in (("i32", 0), ("i8", 0), ("f32", 0), ("f32", 1)):
            assert L.plhip_dw_conv1x1_fused_supported(ctypes.byref(d), m, E.OUT_KINDS[out], tail) == 1, (c["name"], out, tail)
            p = D.plan_of(pkg.capi, c, out, tail)
            assert p["name"] == "dw_conv1x1", (c["name"], p["text"])
            # the output kind and the tail choose the kernel instance, never the tiling
            assert {k: v for k, v in p.items() if k != "text"} == {k: v for k, v in plans[c["name"]].items() if k != "text"}, c["name"]
        p = plans[c["name"]]
        assert p["lds"] <= 64 * 1024 and p["block"] == 256 and p["grid"] == (c["shape"][0] * p["tpi"], p["mgroups"]), p["text"]


def test_every_case_meets_the_classes_it_claims(plans):
    for c in D.CASES:
        assert c["classes"], c["name"]
        for k in c["classes"]:
            assert D.CLASSES[k](plans[c["name"]]), "%s is not in class %s: %s" % (c["name"], k, plans[c["name"]]["text"])
    claimed = {k for c in D.CASES for k in c["classes"]}
    assert claimed == set(D.CLASSES), set(D.CLASSES) - claimed
    # the numbers the issue's table states
    p = plans["wide130"]
    assert (p["ow"], p["tr_tiles"], p["tpi"], p["DWORD"]) == (130, 3, 6, 0)
    assert (plans["s2_wide130"]["ow"], plans["s2_wide256_pl0"]["ow"], plans["s2_128"]["ow"], plans["s2_128"]["cw_tiles"]) == (130, 256, 128, 1)
    assert (plans["halved_s2_ow4"]["TR"], plans["halved_s2_ow4"]["tr_tiles"]) == (16, 3)
    assert (plans["halved_s2_ow5"]["TR"], plans["halved_s1_ow1"]["TR"], plans["halved_s1_ow1"]["CW"]) == (13, 64, 1)
    p = plans["ragged_m264"]
    assert (p["mt32"], p["mtpb"], p["mgroups"], p["NACC"]) == (9, 8, 2, 8)
    assert (plans["ragged_m544"]["mt32"], plans["ragged_m544"]["mtpb"]) == (17, 16)


def test_misaligned_x_turns_dword_rows_into_byte_rows(pkg):
    n = 0
    for c in D.CASES:
        if not c["x_off"]:
            continue
        al, un = D.plan_of(pkg.capi, c, x_aligned=1), D.plan_of(pkg.capi, c, x_aligned=0)
        assert c["shape"][3] % 4 == 0 and c["x_off"] in (1, 2, 3)
        assert al["DWORD"] == 1 and un["DWORD"] == 0 and un["wu"] == al["WP"] == 4 * al["wu"], c["name"]
        assert {k: v for k, v in al.items() if k not in ("DWORD", "wu", "rpp", "text")} == \
               {k: v for k, v in un.items() if k not in ("DWORD", "wu", "rpp", "text")}
        n += 1
    assert n == 6
    assert D.plan_of(pkg.capi, D.BY_NAME["x_off1_wide256"])["wu"] > 64  # every wide byte-staged row takes a second trip


def test_the_table_covers_every_regime(plans):
    ps = list(plans.values())

    def seen(f):
        return {f(p) for p in ps}
    assert seen(lambda p: p["NACC"]) == {1, 2, 4, 8}
    assert seen(lambda p: (p["S"], p["PL"])) == {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert seen(lambda p: p["DWORD"]) == {0, 1}
    assert seen(lambda p: p["cw_tiles"] > 1) == {False, True}
    assert seen(lambda p: "one" if p["mgroups"] == 1 else ("whole" if p["mt32"] % p["mtpb"] == 0 else "ragged")) == {"one", "whole", "ragged"}
    assert seen(lambda p: p["rpp"] > 1) == {False, True}
    assert seen(lambda p: (p["DWORD"], p["wu"] > 64)) == {(0, False), (0, True), (1, False), (1, True)}
    assert seen(lambda p: p["tpi"] > 1) == {False, True}
    assert seen(lambda p: p["oh"] % p["TR"] != 0) == {False, True} and seen(lambda p: p["ow"] % p["CW"] != 0) == {False, True}
    assert seen(lambda p: p["KS"] % 2) == {0, 1} and max(p["KS"] for p in ps) == 32
    # all 16 padding combinations on both strides and both planes
    pads = {(c["shape"][2:4], c["shape"][4], c["shape"][5]) for c in D.CASES if c["group"] == "pads"}
    assert len(pads) == 64
    # the tail, the unaligned outputs and the batch sweep run on the wide, halved, ragged-M-group and PL = 0 regimes
    for k in ("wide", "halved", "ragged_mgroup", "pl0", "bytes", "dword", "wu66"):
        assert any(k in D.BY_NAME[n]["classes"] for n in D.EDGE_CASES), k
    assert {plans[n]["tpi"] > 1 for n in D.BATCH_CASES} == {False, True}
    assert all(D.BY_NAME[n]["shape"][0] >= 2 for n in D.BATCH_CASES)


@pytest.mark.parametrize("name", D.EDGE_CASES)
def test_stated_seeds_reach_every_value_edge(plref, name):
    """Per activation pair the oracle's results lack no edge (dwconv_cases.stage_misses / calib_misses); over the pair, each of
    the depthwise stage, the 1x1 stage and the calib copy of the residual sum shows ties of both signs, both saturation bounds
    with values exactly on +-127.5 (conv stages), the relu6 bound and round-toward-zero fractions."""
    case = D.BY_NAME[name]
    both = {"dw": {}, "pw": {}, "q": {}}
    for j, (act, alpha, _seed) in enumerate(D.acts_of(case)):
        c = D.reference(plref, case, j)
        assert D.case_misses(c, act, alpha) == [], (name, act, alpha)
        assert c["mid"].min() <= -127 or c["dw_act"] != E.ACT_NONE
        stats = {"dw": E.edge_stats(c["pre_mid"], c["dw_act"], c["dw_alpha"]), "pw": E.edge_stats(c["pre"], act, alpha),
                 "q": E.edge_stats(c["tails"]["res"]["pre_q"], E.ACT_NONE, 0.0)}
        stats["q"]["clip"] = E.edge_stats(c["tails"]["calib"]["pre_q"], E.ACT_RELU6, alpha / D.CALIB)["clip"] if act == E.ACT_RELU6 else 0
        for k, st in stats.items():
            for key, v in st.items():
                both[k][key] = both[k].get(key, 0) + v
        for t in c["tails"].values():  # the calib copy is the rounding of pre_q, and it saturates at +-127
            assert np.array_equal(t["q"], np.clip(np.where(t["pre_q"] >= 0, np.floor(t["pre_q"] + 0.5), np.ceil(t["pre_q"] - 0.5)), -127, 127))
    for k, st in both.items():
        for key in ("tie_pos", "tie_neg", "sat_pos", "sat_neg", "clip", "rtz") + (("at_127_5", "at_m127_5") if k != "q" else ()):
            assert st[key] > 0, (name, k, key, st)


def test_every_case_has_distinct_images_and_live_outputs(plref):
    """No case degenerates: the int8 output is not constant, and the images of a batch differ (so a wrong image cannot pass)."""
    for c in D.CASES:
        for j in range(len(D.acts_of(c))):
            r = D.reference(plref, c, j)
            assert r["ref_i8"].shape[:2] == (c["shape"][0], c["shape"][6])
            assert len(np.unique(r["ref_i8"])) > 1 or r["ref_i8"].size <= 16, c["name"]
    for name in D.BATCH_CASES:
        case = D.BY_NAME[name]
        act, alpha, seed = D.acts_of(case)[0]
        r = D.make(plref, case, act, alpha, seed, n=max(D.BATCH_NS))
        assert len({r["ref_i8"][b].tobytes() for b in range(max(D.BATCH_NS))}) == max(D.BATCH_NS)


def test_binding_places_x_y_and_y_i8_and_returns_the_margins(pkg, monkeypatch):
    """Context.dw_conv1x1_fused over the stub library: x lies misalign[0] bytes, y misalign[1] elements and y_i8 misalign[2]
    bytes past a 16-byte boundary, every other operand on one; with a sentinel both allocations come back filled around the
    tensors, and without one the call is what it always was."""
    capi = pkg.capi
    d = capi.conv_desc(1, 16, 4, 4, 16, 3, 3, (1, 1, 1, 1), (1, 1), (1, 1), 16)
    x, wd, wp = np.zeros((1, 16, 4, 4), np.int8), np.zeros((16, 1, 3, 3), np.int8), np.zeros((8, 16, 1, 1), np.int8)
    s1, s2, res = np.ones(16, np.float32), np.ones(8, np.float32), np.zeros((1, 8, 4, 4), np.float32)

    def call(out, **kw):
        ctx, lib = stub_context(capi, monkeypatch)
        r = ctx.dw_conv1x1_fused(d, x, wd, s1, None, wp, s2, None, 0, 0.0, out, **kw)
        assert ctx.outstanding() == 0 and not lib.live
        return r, dict(lib.calls)["plhip_dw_conv1x1_fused_int8"]
    # x, dw_w, dw_scale, dw_bias, packed weights, pw_scale, pw_bias, y, residual, y_i8
    r, res0 = call(capi.OUT_F32, residual=res, calib_scale=0.5)
    assert res0 == [0, 0, 0, None, 0, 0, None, 0, 0, 0] and len(r) == 2
    r, got = call(capi.OUT_F32, residual=res, calib_scale=0.5, misalign=(3, 1, 2), sentinel=0xA5)
    assert got == [3, 0, 0, None, 0, 0, None, 4, 0, 2]
    y, yq, my, mq = r
    assert y.shape == res.shape and yq.shape == res.shape and y.dtype == np.float32 and yq.dtype == np.int8
    assert (y.view(np.uint8) == 0xA5).all() and (yq.view(np.uint8) == 0xA5).all()
    assert my.size == 2 * capi.MARGIN_GUARD + 4 + capi.SCOPE_SLACK and mq.size == 2 * capi.MARGIN_GUARD + 2 + capi.SCOPE_SLACK
    assert (my == 0xA5).all() and (mq == 0xA5).all()
    r, got = call(capi.OUT_I8, misalign=1)
    assert got == [1, 0, 0, None, 0, 0, None, 1, None, None] and r[1] is None
    r, got = call(capi.OUT_F32, calib_scale=0.5, want_y=False, misalign=(0, 3, 3), sentinel=0)
    assert got == [0, 0, 0, None, 0, 0, None, None, None, 3] and r[0] is None and r[2] is None and (r[3] == 0).all()
