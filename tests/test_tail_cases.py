"""CPU guard for test_gpu_conv_tail.py: the case table of tail_cases.py against the library's own launch plans and against the
oracle alone.  Every case reaches the route and the kernel instance it names under default knobs, the table as a whole covers a
stated set of instances, the int8-staged epilogue of gemm_tr is taken for one tail word only, the cases with stated seeds put the
conv output and every calib copy on their value edges, and the fused entry point answers "supported" for every case and not for
the direct 3x3 stride-2 stem.  The binding's misalign / sentinel arguments are checked over test_capi_scope_host.py's stub
library.  Runs without a GPU."""
import ctypes

import numpy as np
import pytest

import dwconv_cases as D
import edge_cases as E
import tail_cases as T
from test_capi_scope_host import stub_context

TAIL_WORDS = {"none": 0, "res": T.TAIL_RES, "calib": T.TAIL_CALIB, "res+calib": T.TAIL_RES | T.TAIL_CALIB,
              "calib, f32 dropped": T.TAIL_CALIB | T.TAIL_NO_F32, "res+calib, f32 dropped": T.TAIL_RES | T.TAIL_CALIB | T.TAIL_NO_F32}


@pytest.fixture(scope="module")
def plans(pkg):
    """name -> the plan of the case's tail launch "residual + calib" under aligned pointers."""
    for k, v in E.KNOB_DEFAULTS.items():
        assert pkg.capi.load().plhip_debug_set(k.encode(), v) == 0
    return {c["name"]: T.plan_of(pkg.capi, c["shape"]) for c in T.CASES}


def test_every_case_reaches_the_route_and_instance_it_names(pkg, plans):
    assert len(T.BY_NAME) == len(T.CASES)
    for c in T.CASES:
        p = plans[c["name"]]
        assert p["impl"] == c["impl"], (c["name"], p["impl"])
        assert p["kernel"] == c["kernel"], (c["name"], p["kernel"], p["text"])
        assert c["family"] in T.FAMILIES
        # no tail word moves a case to another kernel or tiling; only OUT (gemm_tr) may differ
        for word, bits in TAIL_WORDS.items():
            q = T.plan_of(pkg.capi, c["shape"], bits)
            if word == "none" and "wide_eligible" in c["classes"]:
                continue
            same = {k: v for k, v in q.items() if k not in ("text", "OUT")}
            assert same == {k: v for k, v in p.items() if k not in ("text", "OUT")}, (c["name"], word, q["text"])


def test_every_case_meets_the_classes_it_claims(plans):
    for c in T.CASES:
        for k in c["classes"]:
            assert T.CLASSES[k](plans[c["name"]]), "%s is not in class %s: %s" % (c["name"], k, plans[c["name"]]["text"])
    claimed = {k for c in T.CASES for k in c["classes"]}
    assert claimed == set(T.CLASSES), set(T.CLASSES) - claimed
    # numbers the table's comments state
    assert (plans["ring_4x5"]["HWX"], plans["ring_7x7"]["HWX"], plans["nchw_7x7"]["HWX"]) == (20, 49, 52)
    assert plans["im2col_g2_dil2"]["HWX"] == 124 and plans["im2col_g2_dil2"]["oh"] * plans["im2col_g2_dil2"]["ow"] == 121
    assert (plans["stat_a_7x7"]["PWp"], plans["s2_7x7_m65"]["PWp"], plans["s2_18"]["PWp"], plans["stat_a_14"]["PWp"]) == (8, 8, 16, 16)
    assert plans["stat_a_7x7"]["OW"] == plans["stream_a_7x7"]["OW"] == plans["s2_7x7_m65"]["OW"] == 7
    assert plans["tr_s2_ow9"]["ow"] == 9 and plans["tr_m160_ow20"]["HWX"] == 20


def test_the_table_covers_the_stated_instances(pkg, plans):
    assert {p["kernel"] for p in plans.values()} == T.INSTANCES
    # every first-generation GEMM kernel, every gemm_tr block shape default knobs produce (TR_CFG 3), the patch launchers
    for k in ("gemm_nchw", "gemm_vperm_lds", "gemm_ring", "gemm_ring_ma1", "gemm_areg", "gemm_tr_4x1", "gemm_tr_2x2", "gemm_tr_1x4",
              "stem7x7s2", "im2col_g2/gemm_nchw", "im2col_g1/gemm_nchw"):
        assert k in T.INSTANCES
    for launcher in ("patch_stat_a", "patch_stream_a", "patch_s2"):
        assert {launcher + "/local", launcher + "/global"} <= T.INSTANCES
    # the 2 x 2 wave layout exists at two chunks and in local mode only: the other forms are shapes the route declines
    assert "patch_stat_b/local" in T.INSTANCES
    for shape, lands_on in T.DECLINED:
        assert T.plan_of(pkg.capi, shape)["kernel"] == lands_on, shape
    # each family has stated seeds, both vector-store forms and a case whose rows end off a group of four
    for fam in T.FAMILIES:
        assert any(T.BY_NAME[n]["family"] == fam for n in T.EDGE_CASES), fam
        assert any(c["family"] == fam and a == E.ACT_LEAKY for c in T.CASES for a, _al, _s in T.acts_of(c)), fam
        assert any(T.BY_NAME[n]["family"] == fam for n, _a, _al in T.ND_CASES), fam
    assert {plans[n]["VS"] for n in T.EDGE_CASES if T.BY_NAME[n]["family"] == "gemm" and "VS" in plans[n]} == {0, 1}
    assert {T.BY_NAME[n]["impl"] for n in T.BATCH_CASES} == {T.GEMM, T.PATCH, T.IMPLICIT}
    assert plans["stat_a_7x7"]["glob"] == 1
    assert [p["kernel"] for p in (T.plan_of(pkg.capi, T.BY_NAME["stat_a_7x7"]["shape"], n=n) for n in T.BATCH_NS)] == ["patch_stat_a/global"] * 4


def test_gemm_tr_stages_int8_for_one_tail_word_only(pkg, plans):
    """OUT flips to int8 (tr_stage_i8_calib) for "calib, fp32 dropped, no residual" and for nothing else."""
    n = 0
    for c in T.CASES:
        if c["family"] != "tr":
            continue
        for word, bits in TAIL_WORDS.items():
            out = T.plan_of(pkg.capi, c["shape"], bits)["OUT"]
            assert out == (E.OUT_KINDS["i8"] if word == "calib, f32 dropped" else E.OUT_KINDS["f32"]), (c["name"], word)
        n += 1
    assert n >= 6
    for c in T.CASES:  # the other GEMM kernels never flip
        if c["family"] != "tr" and "OUT" in plans[c["name"]]:
            assert {T.plan_of(pkg.capi, c["shape"], b)["OUT"] for b in TAIL_WORDS.values()} == {E.OUT_KINDS["f32"]}, c["name"]


def test_a_tail_keeps_the_wide_kernel_away(pkg):
    capi, shape = pkg.capi, T.BY_NAME["areg_4x8"]["shape"]
    d = T.desc_of(capi, shape)
    assert capi.gemm_plan_text(d, E.OUT_KINDS["i8"], 0).startswith("gemm_wide_")
    for bits in list(TAIL_WORDS.values())[1:]:
        assert capi.gemm_plan_text(d, E.OUT_KINDS["f32"], bits).startswith("gemm_areg "), bits


def test_the_alignment_bit_clears_the_vector_stores(pkg, plans):
    """TAIL_UNALIGNED is what vec_store_ok answers for a pointer off its alignment: VS = 0 (and with it MF of the dword kernels),
    the same kernel and grid."""
    n = 0
    for c in T.CASES:
        p = plans[c["name"]]
        if "VS" not in p:
            continue
        q = T.plan_of(pkg.capi, c["shape"], T.TAIL_RES | T.TAIL_CALIB | T.TAIL_UNALIGNED)
        assert q["VS"] == 0 and q["kernel"] == p["kernel"] and (q["grid"], q["NT"], q["MT"]) == (p["grid"], p["NT"], p["MT"]), c["name"]
        if p["VS"] == 1:
            assert q["MF"] == (p["MF"] if p["family"] == "ring" else 0), c["name"]
            n += 1
    assert n >= 5


def test_patch_plan_text_is_the_launchers_plan(pkg, plans):
    """The fields the kernel's grid and LDS pitch come from, at the values launch_conv_patch computes for the table's shapes."""
    p = plans["stat_a_14"]
    assert (p["name"], p["glob"], p["NCH"], p["TPI"], p["T"], p["T8"], p["MB"], p["NQ"], p["rounds"], p["pitch"]) == \
        ("patch_stat_a", 0, 2, 1, 2, 1, 1, 1, 1, 288)
    p = plans["stat_b_m64"]
    assert (p["name"], p["TPI"], p["MB"], p["pitch"]) == ("patch_stat_b", 1, 1, 480)
    p = plans["stat_a_7x7"]  # global mode: one "image" of 3 x 72 pixels
    assert (p["glob"], p["B"], p["PLANE"], p["TPI"], p["T"]) == (1, 1, 216, 1, 1)
    p = plans["s2_7x7_m65"]
    assert (p["name"], p["glob"], p["NCH"], p["MB"], p["PLANE"]) == ("patch_s2", 1, 4, 1, 192)
    big = T._fields(pkg.capi.patch_plan_text(pkg.capi.conv_desc(4, 64, 56, 56, 64, 3, 3, (1, 1, 1, 1))))
    assert (big["name"], big["TPI"], big["T"], big["T8"], big["rounds"] * big["NQ"] >= big["T8"]) == ("patch_stat_b", 8, 32, 4, True)
    assert pkg.capi.patch_plan_text(T.desc_of(pkg.capi, T.BY_NAME["lds_6x6"]["shape"])) == ""


def test_tail_rejection(pkg):
    L = pkg.capi.load()
    d = T.desc_of(pkg.capi, T.REFUSED_SHAPE)
    assert L.plhip_conv_impl_name(ctypes.byref(d)).decode() == T.DIRECT_S2
    assert L.plhip_conv2d_fused_supported(ctypes.byref(d)) == 0
    for c in T.CASES:
        for n in (None, 1, 9):
            assert L.plhip_conv2d_fused_supported(ctypes.byref(T.desc_of(pkg.capi, c["shape"], n=n))) == 1, c["name"]


@pytest.mark.parametrize("name", T.EDGE_CASES)
def test_stated_seeds_reach_every_value_edge(plref, name):
    """Per activation the oracle's results lack no edge its activation and relu admit; over the pair the conv output shows ties
    of both signs, both saturation bounds with values exactly on +-127.5, the relu6 bound and round-toward-zero fractions, and
    so does the calib copy of the residual sum."""
    case = T.BY_NAME[name]
    both = {"conv": {}, "q": {}}
    for j, (act, alpha, _seed) in enumerate(T.acts_of(case)):
        c = T.reference(plref, case, j)
        assert T.case_misses(c, act, alpha) == [], (name, act, alpha)
        stats = {"conv": E.edge_stats(c["pre"], act, alpha), "q": E.edge_stats(c["tails"]["res"]["pre_q"], E.ACT_NONE, 0.0)}
        stats["q"]["clip"] = E.edge_stats(c["tails"]["calib"]["pre_q"], E.ACT_RELU6, alpha / T.CALIB)["clip"] if act == E.ACT_RELU6 else 0
        for k, st in stats.items():
            for key, v in st.items():
                both[k][key] = both[k].get(key, 0) + v
        for key in D.TAILS:  # the calib copy is the rounding of pre_q, and it saturates at +-127
            t = c["tails"][key]
            assert np.array_equal(t["q"], np.clip(np.where(t["pre_q"] >= 0, np.floor(t["pre_q"] + 0.5), np.ceil(t["pre_q"] - 0.5)), -127, 127))
        assert c["tails"]["res_relu_f32"]["q"] is None and c["tails"]["res_relu_f32"]["z"] is c["tails"]["res_relu"]["z"]
    for k, st in both.items():
        for key in ("tie_pos", "tie_neg", "sat_pos", "sat_neg", "clip", "rtz") + (("at_127_5", "at_m127_5") if k != "q" else ()):
            assert st[key] > 0, (name, k, key, st)


def test_find_seeds_gives_the_stated_seeds(plref):
    for name in T.EDGE_CASES[:3]:
        assert T.find_seeds(plref, T.BY_NAME[name], limit=8) == T.BY_NAME[name]["seeds"], name


def test_every_case_has_distinct_images_and_live_outputs(plref):
    for c in T.CASES:
        for j in range(len(T.acts_of(c))):
            r = T.reference(plref, c, j)
            assert r["pre"].shape[:2] == (c["shape"][0], c["shape"][4])
            assert len(np.unique(r["tails"]["res"]["q"])) > 8, c["name"]
            assert len({r["tails"]["res"]["q"][b].tobytes() for b in range(c["shape"][0])}) == c["shape"][0], c["name"]
    for name, act, alpha in T.ND_CASES:
        r = T.reference_nondyadic(plref, name, act, alpha)
        s = r["scale"].astype(np.float64)
        assert not (np.log2(s) == np.round(np.log2(s))).any() and r["calib"] == T.ND_CALIB
    for name in T.BATCH_CASES:
        case = T.BY_NAME[name]
        act, alpha, seed = T.acts_of(case)[0]
        r = T.make(plref, case, act, alpha, seed, n=max(T.BATCH_NS))
        assert len({r["tails"]["res"]["q"][b].tobytes() for b in range(max(T.BATCH_NS))}) == max(T.BATCH_NS)


def test_binding_places_x_y_residual_and_y_i8_and_returns_the_margins(pkg, monkeypatch):
    """Context.conv2d_fused over the stub library: x lies misalign[0] bytes, y misalign[1] elements, the residual misalign[2]
    elements and y_i8 misalign[3] bytes past a 16-byte boundary, every other operand on one; with a sentinel both allocations
    come back filled around the tensors, and without one the call is what it always was."""
    capi = pkg.capi
    d = capi.conv_desc(1, 16, 4, 4, 8, 1, 1)
    x, w = np.zeros((1, 16, 4, 4), np.int8), np.zeros((8, 16, 1, 1), np.int8)
    sc, res = np.ones(8, np.float32), np.zeros((1, 8, 4, 4), np.float32)

    def call(*a, **kw):
        ctx, lib = stub_context(capi, monkeypatch)
        r = ctx.conv2d_fused(d, x, w, sc, None, *a, **kw)
        assert ctx.outstanding() == 0 and not lib.live
        return r, dict(lib.calls)["plhip_conv2d_int8_fused"]
    # x, packed weights, scale, bias, y, residual, y_i8, workspace
    r, got = call(res, 0, 0.5)
    assert got == [0, 0, 0, None, 0, 0, 0, 0] and len(r) == 2
    r, got = call(res, 1, 0.5, misalign=(3, 1, 2, 3), sentinel=0xA5)
    assert got == [3, 0, 0, None, 4, 8, 3, 0]
    y, yq, my, mq = r
    assert y.shape == res.shape and yq.shape == res.shape and y.dtype == np.float32 and yq.dtype == np.int8
    assert my.size == 2 * capi.MARGIN_GUARD + 4 + capi.SCOPE_SLACK and mq.size == 2 * capi.MARGIN_GUARD + 3 + capi.SCOPE_SLACK
    assert (my == 0xA5).all() and (mq == 0xA5).all() and (yq.view(np.uint8) == 0xA5).all()
    r, got = call(None, 0, 0.5, want_f32=False, misalign=(0, 3, 3, 2), sentinel=0)
    assert got == [0, 0, 0, None, None, None, 2, 0] and r[0] is None and r[2] is None and (r[3] == 0).all()
    r, got = call(res, 1, None, misalign=1)
    assert got == [1, 0, 0, None, 4, 4, None, 0] and r[1] is None
