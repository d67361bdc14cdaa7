"""CPU guard for test_gpu_gemm_instances.py: the case table of gemm_cases.py against the library's own launch plans and against
the oracle alone.  Every case reaches the route and the kernel instance it claims under its knobs, for every output kind,
activation and pointer offset it runs; the claimed instances are exactly the set enumerated from the launchers' dispatch (whose
per-family counts are tools/dump_gemm_plans.INSTANCES) minus UNREACHABLE; every class is claimed in every family it applies to and
holds on the plan; no knob leaks; and the cases with stated seeds put the values the int8 epilogues round on every edge.  Runs
without a GPU."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import edge_cases as E
import gemm_cases as G
import tail_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBES = ((2, 128, 4, 8, 256, 1, T.P0, 1, 1, 1), (2, 24, 9, 16, 128, 5, T.P2, 1, 1, 1), (2, 96, 6, 6, 80, 1, T.P0, 1, 1, 1),
          (2, 160, 4, 5, 200, 1, T.P0, 1, 1, 1))


def _probe(capi):
    return [capi.gemm_plan_text(T.desc_of(capi, s), E.OUT_KINDS[o], t) for s in PROBES for o in G.OUTS for t in (0, 8, 16)]


@pytest.fixture(scope="module")
def lib(pkg):
    L = pkg.capi.load()
    for k, v in E.KNOB_DEFAULTS.items():
        assert L.plhip_debug_set(k.encode(), v) == 0
    pkg.capi.load().plhip_debug_wide_ntt(-1)
    return L


def _reached(capi, L):
    """{key: [what reached it]} over every launch of the table, each asserted to be the key its case claims."""
    reached = {}
    for c in G.CASES:
        with E.Knobs(L, c["knobs"]):
            d = T.desc_of(capi, c["shape"])
            assert L.plhip_conv_impl_name(ctypes.byref(d)).decode() == c["impl"], c["name"]
            for out, act, _alpha, _j in G.launches(c):
                key, f = G.key_of(capi, c["shape"], out, act)
                assert key == G.claimed_key(c, out, act), (c["name"], out, act, f["text"])
                reached.setdefault(key, []).append(c["name"])
    for name, claim_x, claim_y in G.POINTER_CASES:
        c = G.BY_NAME[name]
        with E.Knobs(L, c["knobs"]):
            for mis in G.POINTER_OFFSETS:
                for out in G.OUTS:
                    for act, _alpha, _seed in G.acts_of(c)[:2]:
                        key, f = G.key_of(capi, c["shape"], out, act, G.mis_tail(mis))
                        assert key == G.claimed_key(c, out, act, claim_x if mis[0] else claim_y), (name, mis, out, f["text"])
                        reached.setdefault(key, []).append("%s@x%d,y%d" % ((name,) + mis))
    return reached


def test_the_enumeration_is_the_librarys_instance_count():
    spec = importlib.util.spec_from_file_location("dump_gemm_plans", os.path.join(ROOT, "tools", "dump_gemm_plans.py"))
    dump_gemm_plans = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dump_gemm_plans)
    want = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", dump_gemm_plans.INSTANCES)}
    keys = G.expected_keys()
    without_nonneg = {k[:-1] for k in keys}
    got = {fam: sum(1 for k in without_nonneg if G.plan_family(k) == fam) for fam in want}
    assert got == want == {"private": 24, "lds": 24, "ring": 48, "tr": 30, "wide": 30}, (got, want)
    assert len(keys) == 166 and len(without_nonneg) == 156  # NONNEG splits the wide kernel's 10 int8 instances
    assert len({len(k) for k in keys}) == 1 and len(G.KEY_FIELDS) == 13


def test_every_case_reaches_its_instance_and_the_table_covers_exactly_the_set(pkg, lib):
    before = _probe(pkg.capi)
    assert len(G.BY_NAME) == len(G.CASES) and {c["family"] for c in G.CASES} == set(G.FAMILIES)
    reached = _reached(pkg.capi, lib)
    expected = G.expected_keys()
    assert set(G.UNREACHABLE) <= expected and all(isinstance(why, str) and ":" in why for why in G.UNREACHABLE.values())
    assert set(reached) == G.table_keys()
    assert set(reached) == expected - set(G.UNREACHABLE), (sorted(expected - set(G.UNREACHABLE) - set(reached)), sorted(set(reached) - expected))
    for fam in G.FAMILIES:
        n_exp = sum(1 for k in expected if G.test_family(k) == fam)
        n_got = sum(1 for k in reached if G.test_family(k) == fam)
        print("%-8s claimed %3d of %3d enumerated" % (fam, n_got, n_exp))
        assert n_got == n_exp - sum(1 for k in G.UNREACHABLE if G.test_family(k) == fam)
    print("UNREACHABLE:", G.UNREACHABLE or "none")
    assert len(G.UNREACHABLE) <= 8
    # shapes stay tiny
    for c in G.CASES:
        n, cin, h, w, cout, k = c["shape"][:6]
        assert n <= 3 and h <= 14 and w <= 22 and cout <= 320 and cin * k * k <= 1024, c["name"]
        oh, ow = pkg.capi.out_hw(T.desc_of(pkg.capi, c["shape"]))
        assert oh <= 8 and ow <= 20, c["name"]
    assert _probe(pkg.capi) == before  # no knob leaked


def test_every_knob_the_table_uses_has_its_default(pkg, lib):
    used = {k for c in G.CASES for k in c["knobs"]}
    assert used == {"GEMM_VARIANT", "GEMM_AREG", "GEMM_MA", "GEMM_TR", "TR_CFG", "GEMM_WIDE", "WIDE_NTT"} and used <= set(E.KNOB_DEFAULTS)
    assert (E.KNOB_DEFAULTS["GEMM_TR"], E.KNOB_DEFAULTS["TR_CFG"], E.KNOB_DEFAULTS["GEMM_WIDE"]) == (1, 3, 1)
    assert {c["knobs"]["TR_CFG"] for c in G.CASES if "TR_CFG" in c["knobs"]} | {3} == {0, 1, 2, 3}
    # GEMM_MA = 1 is the other way to 32-row wave tiles: without it the same shape runs 64-row ones
    c = G.BY_NAME["r1_ks5_m192_forced"]
    with E.Knobs(lib, G.RING):
        assert G.key_of(pkg.capi, c["shape"], "i8")[0] == G.make_key("ring", "i8", MA=2, VS=1, MF=1)
    # and plhip_debug_wide_ntt the other way to a forced wide tile
    w = G.BY_NAME["w7_ks8_m256_4x4"]
    before = _probe(pkg.capi)
    lib.plhip_debug_wide_ntt(7)
    try:
        assert G.key_of(pkg.capi, w["shape"], "f32")[0] == G.claimed_key(w, "f32")
    finally:
        lib.plhip_debug_wide_ntt(-1)
    assert _probe(pkg.capi) == before
    # without a forced tile a 32-bit output stays off the wide kernel, and a plain GEMM off gemm_tr
    assert G.key_of(pkg.capi, w["shape"], "f32")[1]["family"] == "ring"
    assert G.key_of(pkg.capi, G.BY_NAME["tp_2x2_k270_4x5"]["shape"], "i8")[1]["family"] != "tr"
    with E.Knobs(lib, G.TRP):  # "not_wide": GEMM_WIDE = 0 is what keeps the wide kernel off this shape
        assert G.key_of(pkg.capi, G.BY_NAME["tp_1x4_ks4_m256"]["shape"], "i8")[1]["family"] == "wide"


def test_every_case_meets_the_classes_it_claims(pkg, lib):
    for c in G.CASES:
        with E.Knobs(lib, c["knobs"]):
            p = G.plan_of(pkg.capi, c)
        for k in c["classes"]:
            assert G.CLASSES[k](p), "%s is not in class %s: %s" % (c["name"], k, p["text"])
    assert {k for c in G.CASES for k in c["classes"]} == set(G.CLASSES)
    assert set(G.FAMILY_CLASSES) == set(G.FAMILIES)
    for fam, classes in G.FAMILY_CLASSES.items():
        have = {k for c in G.CASES if c["family"] == fam for k in c["classes"]}
        assert set(classes) <= have, (fam, set(classes) - have)
    # numbers the table's comments state: ring depths, the K-steps of the implicit shapes
    with E.Knobs(lib, {"TR_CFG": 0}):
        assert G.plan_of(pkg.capi, G.BY_NAME["ti_4x2_ks5_ow16"])["D"] == 4
    assert G.plan_of(pkg.capi, G.BY_NAME["ti_2x2_ks5_ow9"])["D"] == 3
    assert [G.plan_of(pkg.capi, G.BY_NAME[n])["ksteps"] for n in ("ti_4x1_ks4_ow7", "ti_2x2_ks5_ow9", "ti_1x4_ks7_ow20",
                                                                   "ti_4x1_ks13_ow16", "ti_2x2_ks19_s2")] == [4, 5, 7, 13, 19]


def test_the_pointer_sweep_and_the_side_tables_name_every_family(pkg, lib):
    fams = lambda names: {G.BY_NAME[n]["family"] for n in names}
    assert fams(n for n, _x, _y in G.POINTER_CASES) == set(G.FAMILIES)
    assert fams(G.EDGE_CASES) == fams(G.BATCH_CASES) == fams(G.MAXMAG_CASES) == fams(n for n, _a, _al in G.ND_CASES) == set(G.FAMILIES)
    assert G.POINTER_OFFSETS == ((1, 0), (3, 0), (0, 1), (0, 2), (0, 3))
    for name in G.MAXMAG_CASES:  # the family's largest K in the table
        c = G.BY_NAME[name]
        kof = lambda q: q["shape"][1] * q["shape"][5] ** 2
        assert kof(c) == max(kof(q) for q in G.CASES if q["family"] == c["family"]), name
    for name in G.BATCH_CASES:  # the instance does not depend on the batch
        c = G.BY_NAME[name]
        with E.Knobs(lib, c["knobs"]):
            assert {G.key_of(pkg.capi, c["shape"], "i8", n=n)[0] for n in G.BATCH_NS} == {G.claimed_key(c, "i8")}, name
    # every int8 activation template on every family: requant4<none / relu / relu6 / leaky>, the wide kernel's NONNEG 0 and 1
    for fam in G.FAMILIES:
        acts = {a for c in G.CASES if c["family"] == fam and c["seeds"] for a, _al, _s in G.acts_of(c)}
        assert acts == {E.ACT_NONE, E.ACT_RELU, E.ACT_RELU6, E.ACT_LEAKY}, fam
    for c in G.CASES:
        assert {G.nonneg(a) for a, _al, _s in G.acts_of(c)} == {0, 1}, c["name"]


@pytest.mark.parametrize("name", G.EDGE_CASES)
def test_stated_seeds_reach_every_value_edge(plref, name):
    """From the oracle alone: per activation no edge it admits is missing, and over the seven activations the values the int8
    output rounds show ties of both signs, values on +-127.5 and past both bounds, the relu6 bound hit for an integer, a
    half-integer and a bound above 127, and ties among the leaky products."""
    case = G.BY_NAME[name]
    assert len(case["seeds"]) == len(E.ACTS)
    total, clips, leaky = {}, {}, 0
    for j, (act, alpha, _seed) in enumerate(G.acts_of(case)):
        c = G.reference(plref, case, j)
        assert G.case_misses(c, act, alpha) == [], (name, act, alpha)
        st = E.edge_stats(c["pre"], act, alpha)
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
        if act == E.ACT_RELU6:
            clips[alpha] = st["clip"]
        if act == E.ACT_LEAKY:
            leaky += G.leaky_ties(c)
        # the int8 reference is the rounding of pre (half away from zero), saturated at +-127
        pre = c["pre"].astype(np.float64)
        assert np.array_equal(c["ref_i8"], np.clip(np.where(pre >= 0, np.floor(pre + 0.5), np.ceil(pre - 0.5)), -127, 127))
    for k in ("tie_pos", "tie_neg", "at_127_5", "at_m127_5", "sat_pos", "sat_neg", "rtz"):
        assert total[k] > 0, (name, k, total)
    assert set(clips) == {60.0, 60.5, 200.5} and all(v > 0 for v in clips.values()), (name, clips)
    assert leaky > 0, name
    print("%s: %s relu6 bound hits %s leaky ties %d" % (name, {k: v for k, v in total.items() if k != "n"}, clips, leaky))


def test_find_seeds_gives_the_stated_seeds(plref):
    for name in G.EDGE_CASES[:3]:
        assert G.find_seeds(plref, G.BY_NAME[name], limit=8) == G.BY_NAME[name]["seeds"], name


def test_operands_are_what_the_gpu_test_needs(plref):
    """Distinct images in every batch sweep, scales that are no powers of two in the non-dyadic sets, -128 and accumulators of
    full magnitude in the maximum-magnitude ones."""
    for name in G.BATCH_CASES:
        case = G.BY_NAME[name]
        act, alpha, seed = G.acts_of(case)[0]
        r = G.make(plref, case, act, alpha, seed, n=max(G.BATCH_NS))
        assert len({r["ref_i8"][b].tobytes() for b in range(max(G.BATCH_NS))}) == max(G.BATCH_NS), name
    for name, act, alpha in G.ND_CASES:
        r = G.make_nondyadic(plref, G.BY_NAME[name], act, alpha)
        s = r["scale"].astype(np.float64)
        assert not (np.log2(s) == np.round(np.log2(s))).any() and len(np.unique(r["ref_i8"])) >= 6, name
    for name in G.MAXMAG_CASES:
        case = G.BY_NAME[name]
        r = G.make(plref, case, E.ACT_NONE, 0.0, 7000, maxmag=True)
        k = case["shape"][1] * case["shape"][5] ** 2
        # (the implicit shapes' border outputs see padding: the interior reaches K * 127^2)
        assert r["x"].min() == -128 and np.abs(r["acc"].astype(np.int64)).max() >= k * 127 * 127, name
