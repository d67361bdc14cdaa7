"""What the launch-graph tests share (tests/test_gpu_replay.py, the replay checks of the whole-program suites): which device variables
a plan writes, which of them a replay does not rewrite by design, how to fill the rest with the poison byte, how to give a recorded
graph new input, and the one check every program goes through: a REPLAY on input that only the replay ever saw, into poisoned
variables, equals the plain run of a second predictor byte for byte.

The host part (written / feeds / once_outputs / keep) reads plan lines only and is checked on the CPU by
tests/test_replay_cases_host.py."""
import ctypes as C
import time

import numpy as np

POISON = 0xA5  # the project's poison byte (capi.DeviceScope fills with it)


def _fields(line):
    """(head, [bare tokens], {key: value}) of a plan line."""
    toks = line.split(" ")
    return toks[0], toks[1:], dict(f.split("=", 1) for f in toks[1:] if "=" in f)


def _outs(kv):
    return kv["out"].split(",")


def written(plan):
    """The device variables a plan writes, read off its lines: every out= (each name of a list; not behind -f32, not the host copy),
    every +calib=, and the +hi= half of a shuffle unit."""
    names = set()
    for l in plan:
        head, toks, kv = _fields(l)
        if head == "io_copy/device_to_host":
            continue
        if "-f32" not in toks:
            names.update(_outs(kv))
        for key in ("+calib", "+hi"):
            if key in kv:
                names.add(kv[key])
    return names


def feeds(plan):
    """([device-side output of every io_copy/host_to_device line], [the instruction indices of those lines])."""
    names, at = [], []
    for i, l in enumerate(plan):
        head, _, kv = _fields(l)
        if head == "io_copy/host_to_device":
            names.append(kv["out"])
            at.append(i)
    return names, at


def _aliases(plan, roots, is_alias):
    """`roots` and, in plan order, the outputs of the lines is_alias(i, head) accepts whose input is already in the set."""
    kept = list(roots)
    for i, l in enumerate(plan):
        head, _, kv = _fields(l)
        if is_alias(i, head) and kv["in"] in kept and kv["out"] not in kept:
            kept.append(kv["out"])
    return kept


def once_outputs(plan):
    """From the plan alone: the outputs of the ops the predictor computes on the host once per shape (prior_box) and the reshape
    aliases of them.  The count a test holds keep() against."""
    roots = [n for l in plan if _fields(l)[0].startswith("prior_box/") for n in _outs(_fields(l)[2])]
    return _aliases(plan, roots, lambda i, head: head.startswith("reshape/"))


def keep(plan, kernel_names):
    """The variables a replay does not rewrite by design, so they may not be poisoned: the feeds' device tensors (the graph leaves the
    io_copy instructions out), the outputs of the instructions whose device function is named *_once (prior_box_host_once: made on
    the host at the first run of a shape) and the reshape_share aliases of either.  From the kernel names the predictor reports, one
    per plan line."""
    assert len(kernel_names) == len(plan), (len(kernel_names), len(plan))
    func = [k.split(" -> ")[-1] for k in kernel_names]
    roots = list(feeds(plan)[0])
    for i, l in enumerate(plan):
        if func[i].endswith("_once"):
            roots += [n for n in _outs(_fields(l)[2]) if n not in roots]
    return _aliases(plan, roots, lambda i, head: func[i] == "reshape_share")


def to_poison(plan, kernel_names):
    """(sorted names to poison and compare, kept names); asserts the kept count against the plan: no variable is skipped quietly."""
    kept = keep(plan, kernel_names)
    feed_side = _aliases(plan, feeds(plan)[0], lambda i, head: head.startswith("reshape/"))  # the feeds and the aliases of them
    assert len(kept) == len(set(kept)) == len(feed_side) + len(once_outputs(plan)), (kept, feed_side, once_outputs(plan))
    return sorted(written(plan) - set(kept)), kept


# ------------------------------------------------------------------ device part
def var_bytes(p, name):
    """The variable's bytes as a flat uint8 array, its full byte size (Predictor.get_var shapes by elements; this does not)."""
    nb = C.c_int64()
    for cap in (1 << 24, 1 << 30):
        buf = np.empty(cap, np.uint8)
        rc = p.L.pllite_get_var(p.h, name.encode(), buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(nb), None, None)
        if rc == 0 or "too small" not in p.L.pllite_last_error().decode():
            break
    p._ck(rc)
    return buf[:nb.value].copy()


def read_bytes(p, names):
    """name -> the variable's bytes."""
    return {n: var_bytes(p, n) for n in names}


def poison(p, ctx, names, sizes=None):
    """Fills every variable with the poison byte over its full byte size (sizes: name -> bytes, else asked of get_var) through
    plhip_memset on `ctx`'s stream: the predictor's stream is drained first, ctx's after.  Reads the largest variable back."""
    names = list(names)
    assert names
    if sizes is None:
        sizes = {n: var_bytes(p, n).size for n in names}
    p.sync()
    for n in names:
        ptr = p.device_ptr(n)
        assert ptr and sizes[n] > 0, n + ": no device memory to poison"
        ctx.check(ctx.L.plhip_memset(ctx.h, C.c_void_p(ptr), POISON, sizes[n]), "memset " + n)
    ctx.sync()
    probe = max(names, key=lambda n: sizes[n])
    got = var_bytes(p, probe)
    assert got.size == sizes[probe] and (got == POISON).all(), probe + ": the poison did not arrive"


def upload_feed(p, name, arr, index):
    """New input for a recorded graph: the host tensor, then the feed's io_copy instruction alone (hip_predictor.h: "new input is a
    plain copy into the feed's device tensor")."""
    p.set_input(name, arr)
    p.run_instruction(index)


def first_difference(plan, got, want):
    """The first variable in plan order whose bytes differ, with the count; None if all are equal."""
    order = []
    for l in plan:
        _, _, kv = _fields(l)
        order += _outs(kv) + [kv[k] for k in ("+calib", "+hi") if k in kv]
    for n in [n for n in order if n in want] + sorted(set(want) - set(order)):
        if got[n].shape != want[n].shape:
            return "%s: %d bytes, the plain run has %d" % (n, got[n].size, want[n].size)
        bad = int((got[n] != want[n]).sum())
        if bad:
            return "%s: %d of %d bytes differ (%d of them still the poison)" % (n, bad, want[n].size, int(((got[n] != want[n]) & (got[n] == POISON)).sum()))
    return None


def build(lite, wl, net, batch, **emit_kw):
    """A predictor with the net lowered; (predictor, plan).  The caller closes it."""
    p = lite.Predictor(0)
    try:
        wl.emit_graph(p, net, batch, **emit_kw)
        plan = p.graph_plan()
        p.graph_lower()
        assert p.num_instructions() == len(plan)
        return p, plan
    except Exception:
        p.close()
        raise


def replay_equals_plain_run(lite, wl, ctx, net, feeds_a, feeds_b, what, must_run=(), probe=None, **emit_kw):
    """feeds_a / feeds_b: host feed name -> array (the batch is the arrays' first dimension).  Predictor R runs feeds_b plainly;
    predictor P records on feeds_a, gets feeds_b through the io_copy instructions alone, has every written variable poisoned, and
    must reproduce R byte for byte in a replay, and in a second one after a second poisoning.  must_run: fragments that must appear
    in P's kernel names; probe: the variable that must differ between feeds_a and feeds_b and after the poisoning (default: the
    network's output).  Prints the kept variables, the count compared and the time; returns (kernel names, plan)."""
    t0 = time.time()
    batch = next(iter(feeds_a.values())).shape[0]
    out = probe or net["output"]
    r, plan = build(lite, wl, net, batch, **emit_kw)
    try:
        # 1. the reference: a plain run on feeds_b
        for k, v in feeds_b.items():
            r.set_input(k, v)
        r.run()
        r.sync()
        names, kept = to_poison(plan, r.kernel_names())
        assert out in names, out
        want = read_bytes(r, names)
        sizes = {n: want[n].size for n in names}
        p, plan_p = build(lite, wl, net, batch, **emit_kw)
        try:
            assert plan_p == plan
            # 2. record on feeds_a
            for k, v in feeds_a.items():
                p.set_input(k, v)
            p.run()
            p.run_graph()  # records, then launches
            p.sync()
            kernels = p.kernel_names()
            assert kernels == r.kernel_names()
            text = "\n".join(kernels)
            for frag in must_run:
                assert frag in text, (frag, text)
            first = var_bytes(p, out)
            assert first.shape == want[out].shape and not np.array_equal(first, want[out]), "feeds_a and feeds_b give the same " + out
            # 3. feeds_b reaches P's device tensors through the io_copy instructions alone; no run() follows
            host_names = {_fields(plan[i])[2]["in"]: i for i in feeds(plan)[1]}
            assert sorted(host_names) == sorted(feeds_b), (sorted(host_names), sorted(feeds_b))
            for k, v in feeds_b.items():
                upload_feed(p, k, v, host_names[k])
            for round_ in (1, 2):
                # 4. poison; the comparison below can fail
                poison(p, ctx, names, sizes)
                assert not np.array_equal(var_bytes(p, out), want[out]), out + " equals the plain run before the replay"
                # 5. / 6. the replay
                p.run_graph()
                p.sync()
                diff = first_difference(plan, read_bytes(p, names), want)
                assert diff is None, "%s, replay %d differs from the plain run, first in plan order: %s" % (what, round_, diff)
            print("%s: kept %s; %d variables (%d bytes) poisoned and compared, twice; %.1f s" % (
                what, kept, len(names), sum(sizes.values()), time.time() - t0))
            return kernels, plan
        finally:
            p.close()
    finally:
        r.close()
