"""GPU: every GEMM kernel instance behind csrc/gemm_plan.h on its value edges, on the cases of gemm_cases.py (test_gemm_cases.py
proves on the host that the table covers exactly the instances the library builds and that the operands reach their edges).

One test per family: private, lds, ring, areg, tr_im, tr_plain, wide.  Every launch first asserts that the library's plan under
the case's knobs is the instance the case claims, runs through Context.conv2d and is compared with plref.conv2d_acc +
plref.epilogue.  With dyadic operands int32, int8 and fp32 outputs are compared bit for bit (both sides do one fmaf on the same
operands: test_gpu_edges.py); one non-dyadic operand set per family holds fp32 to rtol 1e-5 and int8 to the oracle's, one
maximum-magnitude set runs at the family's largest K.  A pointer sweep puts x 1 and 3 bytes and y 1, 2, 3 elements off their
alignment, a batch sweep runs 1, 2, 3 and 9 distinct images.  Every output lies in an allocation filled with 0xA5 whose margins
must come back untouched and of which nothing may be left inside the tensor, so a value stored outside the tensor, or not stored
at all, cannot pass.  The instance keys that ran are collected and held to the table's."""
import ctypes

import numpy as np
import pytest

import edge_cases as E
import gemm_cases as G
import tail_cases as T

pytestmark = pytest.mark.gpu
POISON = 0xA5
RAN = {}  # family -> the keys its test launched
REF = {"i32": "acc", "f32": "ref_f32", "i8": "ref_i8"}


def _eq(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = (got.view(np.uint32) != want.view(np.uint32)) if got.dtype == np.float32 else (got != want)
    assert not bad.any(), "%s: %d of %d differ, first at %s: got %s want %s" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:6], want[bad][:6])


def _launch(ctx, capi, case, c, out, act, alpha, what, mis=(0, 0), claim=None, lo=None, hi=None, exact=True):
    """One launch of images lo..hi of a made case into a poisoned, guarded output; the plan's key asserted first.  Returns y
    after it was found equal to the oracle's (exact), its margins untouched and no poison inside it."""
    x = c["x"][lo:hi]
    d = T.desc_of(capi, case["shape"], act, alpha, n=x.shape[0])
    key, f = G.key_of(capi, case["shape"], out, act, G.mis_tail(mis), n=x.shape[0])
    assert key == G.claimed_key(case, out, act, claim), (what, f["text"])
    assert ctx.L.plhip_conv_impl_name(ctypes.byref(d)).decode() == case["impl"], what
    sc, bi = (None, None) if out == "i32" else (c["scale"], c["bias"])
    y, margins = ctx.conv2d(d, x, c["w"], sc, bi, E.OUT_KINDS[out], misalign=mis, sentinel=POISON)
    assert (margins == POISON).all(), "%s: %d bytes written outside y" % (what, (margins != POISON).sum())
    if exact:
        _eq(y, c[REF[out]][lo:hi], what)
    if out == "i8":  # 0xA5 is the legitimate value -91: none of the fill where the oracle has another value
        left = (y.view(np.uint8) == POISON) & (c["ref_i8"][lo:hi] != np.int8(POISON - 256))
        assert not left.any(), "%s: %d poison bytes left inside y" % (what, left.sum())
    else:
        assert not (y.view(np.uint32) == 0x01010101 * POISON).any(), what + ": poison left inside y"
    RAN.setdefault(case["family"], set()).add(key)
    return y


def _table_launches(ctx, capi, plref, case):
    for out, act, alpha, j in G.launches(case):
        c = G.reference(plref, case, j)
        what = "%s %s act %d alpha %g" % (case["name"], out, act, alpha)
        _launch(ctx, capi, case, c, out, act, alpha, what)


def _pointer_sweep(ctx, capi, plref, case, claim_x, claim_y):
    for mis in G.POINTER_OFFSETS:
        for out in G.OUTS:
            for j, (act, alpha, _seed) in enumerate(G.acts_of(case)[:2]):
                if out == "i32" and j:
                    continue
                c = G.reference(plref, case, j)
                what = "%s %s act %d, x off by %d bytes, y by %d elements" % ((case["name"], out, act) + mis)
                _launch(ctx, capi, case, c, out, act, alpha, what, mis=mis, claim=claim_x if mis[0] else claim_y)


def _nondyadic(ctx, capi, plref, case, act, alpha):
    c = G.make_nondyadic(plref, case, act, alpha)
    what = "%s act %d alpha %g, non-dyadic" % (case["name"], act, alpha)
    y = _launch(ctx, capi, case, c, "f32", act, alpha, what, exact=False)
    np.testing.assert_allclose(y, c["ref_f32"], rtol=1e-5, atol=0, err_msg=what)
    _launch(ctx, capi, case, c, "i8", act, alpha, what + " int8")


def _max_magnitude(ctx, capi, plref, case):
    for j, (act, alpha) in enumerate(((E.ACT_NONE, 0.0), (E.ACT_LEAKY, 0.375))):
        c = G.make(plref, case, act, alpha, 7000 + j, maxmag=True)
        for out in G.OUTS:
            what = "%s %s act %d, maximum magnitude" % (case["name"], out, act)
            _launch(ctx, capi, case, c, out, act, alpha, what)


def _batch_sweep(ctx, capi, plref, case):
    """n in 1, 2, 3, 9 of nine distinct images: every image of every batch equals the oracle's image (_launch) and its own
    batch-1 run."""
    act, alpha, seed = G.acts_of(case)[0]
    big = max(G.BATCH_NS)
    c = G.make(plref, case, act, alpha, seed, n=big)
    assert len({c["ref_i8"][b].tobytes() for b in range(big)}) == big
    for out in ("i8", "f32"):
        def run(lo, hi):
            return _launch(ctx, capi, case, c, out, act, alpha, "%s %s images %d..%d" % (case["name"], out, lo, hi - 1), lo=lo, hi=hi)
        singles = [run(b, b + 1) for b in range(big)]
        for n in G.BATCH_NS:
            got = run(0, n)
            for b in range(n):
                _eq(got[b], singles[b][0], "%s %s n=%d image %d against its batch-1 run" % (case["name"], out, n, b))


@pytest.mark.parametrize("family", G.FAMILIES)
def test_every_instance_of_the_family_on_its_edges(gpu_ctx, pkg, plref, family):
    capi = pkg.capi
    lib = capi.load()
    RAN[family] = set()
    for case in G.CASES:
        if case["family"] != family:
            continue
        with E.Knobs(lib, case["knobs"]):
            _table_launches(gpu_ctx, capi, plref, case)
            for name, claim_x, claim_y in G.POINTER_CASES:
                if name == case["name"]:
                    _pointer_sweep(gpu_ctx, capi, plref, case, claim_x, claim_y)
            for name, act, alpha in G.ND_CASES:
                if name == case["name"]:
                    _nondyadic(gpu_ctx, capi, plref, case, act, alpha)
            if case["name"] in G.MAXMAG_CASES:
                _max_magnitude(gpu_ctx, capi, plref, case)
            if case["name"] in G.BATCH_CASES:
                _batch_sweep(gpu_ctx, capi, plref, case)
    want = {k for k in G.table_keys() if G.test_family(k) == family}
    assert RAN[family] == want, (sorted(want - RAN[family]), sorted(RAN[family] - want))
    print("%s: %d instances on their edges" % (family, len(want)))


def test_the_keys_that_ran_are_the_tables():
    """Over the families whose test ran in this process: the keys launched are the table's, and the table's are the enumerated
    set (so a dispatch change cannot drop an instance unnoticed)."""
    assert G.table_keys() == G.expected_keys() - set(G.UNREACHABLE)
    assert RAN, "no family ran"
    for family, ran in RAN.items():
        assert ran == {k for k in G.table_keys() if G.test_family(k) == family}, family
    print("instance keys executed: %d of %d" % (len(set().union(*RAN.values())), len(G.expected_keys())))
