"""capi.DeviceScope and the whole-op helpers built on it, without a device: Context runs over a stub library whose device
memory is host memory.  The stub records, for every call that reaches the library, each pointer argument modulo 16: the kernels
choose their vector or scalar path by it, so the helpers must place every operand where they always did."""
import ctypes as C

import numpy as np
import pytest

F32 = np.float32


class StubLib:
    """Stands in for libplhip.so.  plhip_malloc hands out 16-byte-aligned host memory, the copies and memset act on it (and
    must stay inside one live allocation), plhip_free records the address.  Size queries return 32, *_supported 1; every
    other plhip_* symbol records its pointer arguments' residues and returns 0, or 1 when its name is in `fail`."""

    def __init__(self, fail=()):
        self.live, self.freed, self.calls, self.copies, self.fail = {}, [], [], 0, set(fail)

    def _inside(self, p, n):
        addr = p.value if isinstance(p, C.c_void_p) else C.cast(p, C.c_void_p).value
        assert any(a <= addr and addr + n <= a + size for a, (_raw, size) in self.live.items()), "copy outside an allocation"

    def plhip_malloc(self, _h, nbytes, ref):
        assert nbytes >= 1
        raw = C.create_string_buffer(nbytes + 16)
        addr = (C.addressof(raw) + 15) & ~15
        self.live[addr] = (raw, nbytes)
        ref._obj.value = addr
        return 0

    def plhip_free(self, _h, p):
        del self.live[p.value]
        self.freed.append(p.value)
        return 0

    def plhip_memcpy_h2d(self, _h, dst, src, n):
        self._inside(dst, n)
        self.copies += 1
        C.memmove(dst, src, n)
        return 0

    def plhip_memcpy_d2h(self, _h, dst, src, n):
        self._inside(src, n)
        C.memmove(dst, src, n)
        return 0

    def plhip_memset(self, _h, p, value, n):
        self._inside(p, n)
        C.memset(p, value, n)
        return 0

    def plhip_last_error(self, _h):
        return b"stub refusal"

    def plhip_deconv_out_dims(self, dref, oh, ow):
        c = dref._obj.conv
        oh._obj.value = (c.h - 1) * c.stride[0] + c.kh - c.pad[0] - c.pad[1]
        ow._obj.value = (c.w - 1) * c.stride[1] + c.kw - c.pad[2] - c.pad[3]
        return 0

    @staticmethod
    def _residue(a):
        if isinstance(a, C.c_void_p):
            return a.value % 16 if a.value else None
        return [v % 16 if v else None for v in a]

    def __getattr__(self, name):
        if not name.startswith("plhip_"):
            raise AttributeError(name)
        if name.endswith("_bytes"):
            return lambda *a: 32
        if name.endswith("_supported"):
            return lambda *a: 1

        def entry(_h, *args):
            ptrs = [a for a in args if a is None or isinstance(a, C.c_void_p) or (isinstance(a, C.Array) and a._type_ is C.c_void_p)]
            self.calls.append((name, [None if a is None else self._residue(a) for a in ptrs]))
            return int(name in self.fail)
        return entry


def stub_context(capi, monkeypatch, fail=()):
    lib = StubLib(fail)
    monkeypatch.setattr(capi, "_lib", lib)  # load() of the host-only helpers (deconv_out_hw)
    ctx = capi.Context.__new__(capi.Context)
    ctx.L, ctx.h, ctx._allocs = lib, C.c_void_p(1), []
    return ctx, lib


@pytest.fixture
def stub(pkg, monkeypatch):
    return stub_context(pkg.capi, monkeypatch)


# ------------------------------------------------------------------ 1. frees on an exception
def test_scope_frees_on_an_exception(stub):
    ctx, lib = stub
    keep = ctx.malloc(8)
    before = ctx.outstanding()
    with pytest.raises(ZeroDivisionError):
        with ctx.scope() as s:
            s.put(np.arange(5, dtype=F32)), s.put(np.arange(3), np.int8, off=1), s.put(np.zeros((2, 2), F32))
            s.out((4,), F32)
            assert ctx.outstanding() == before + 4
            1 / 0
    assert ctx.outstanding() == before and len(lib.freed) == 4 and keep.value in lib.live
    ctx.free_all()
    assert ctx.outstanding() == 0 and not lib.live


def _refused_calls(capi):
    x = np.arange(60, dtype=F32).reshape(1, 4, 3, 5)
    d = capi.conv_desc(1, 16, 4, 4, 16, 1, 1)
    return {
        "plhip_hard_act_f32": lambda ctx: ctx.hard_act(capi.HARD_SWISH, x, mode="both", misalign=1),
        "plhip_conv2d_int8": lambda ctx: ctx.conv2d(d, np.zeros((1, 16, 4, 4), np.int8), np.zeros((16, 16, 1, 1), np.int8),
                                                    np.ones(16, F32), np.zeros(16, F32), capi.OUT_I8),
        "plhip_concat_calib_f32": lambda ctx: ctx.concat_calib([x, x], 1, 0.5, misalign=1),
        "plhip_yolo_head_f32": lambda ctx: ctx.yolo_head([np.zeros((1, 14, 2, 2), F32)] * 2, np.array([[64, 64]], np.int32),
                                                         [[10, 13, 16, 30]] * 2, 2, 0.01, [32, 16]),
    }


@pytest.mark.parametrize("entry", ["plhip_hard_act_f32", "plhip_conv2d_int8", "plhip_concat_calib_f32", "plhip_yolo_head_f32"])
def test_helpers_free_when_the_library_refuses(pkg, monkeypatch, entry):
    ctx, lib = stub_context(pkg.capi, monkeypatch, fail=[entry])
    with pytest.raises(pkg.capi.PlhipError, match="stub refusal"):
        _refused_calls(pkg.capi)[entry](ctx)
    assert lib.calls[-1][0] == entry
    assert ctx.outstanding() == 0 and not lib.live and lib.freed


# ------------------------------------------------------------------ 2. placement and round trip
@pytest.mark.parametrize("off", [0, 1, 4, 15])
def test_scope_places_operands_off_a_16_byte_boundary(stub, off):
    ctx, _lib = stub
    arr = np.arange(7, dtype=np.int16)
    with ctx.scope() as s:
        p = s.put(arr, off=off)
        o = s.out((3, 2), F32, off=off)
        assert p.value % 16 == off and o.ptr.value % 16 == off
        assert np.array_equal(ctx.to_host(p, arr.shape, arr.dtype), arr)
        assert s.put(arr, np.float64, off).value % 16 == off
        assert o.get().shape == (3, 2) and o.get().dtype == F32 and o.margins().size == off + 64


def test_scope_out_round_trip_and_margins(stub):
    ctx, _lib = stub
    pattern = np.arange(10, dtype=np.int32).reshape(2, 5) * 0x01010101
    with ctx.scope() as s:
        o = s.out(pattern.shape, np.int32, off=3, fill=0xA5, guard=64)
        assert o.ptr.value % 16 == 3
        assert (o.get().view(np.uint8) == 0xA5).all()
        C.memmove(o.ptr, pattern.ctypes.data, pattern.nbytes)
        assert np.array_equal(o.get(), pattern)
        m = o.margins()
        assert m.dtype == np.uint8 and m.size == 2 * 64 + 3 + 64 and (m == 0xA5).all()


# ------------------------------------------------------------------ 3. empty and optional operands
def test_scope_empty_and_optional_operands(stub):
    ctx, lib = stub
    with ctx.scope() as s:
        p = s.put_opt(None, F32)
        assert isinstance(p, C.c_void_p) and not p.value and ctx.outstanding() == 0
        assert s.put_opt(np.ones(3), F32).value and ctx.outstanding() == 1
        copies = lib.copies
        e = s.put(np.zeros((0, 4), F32))
        assert e.value and ctx.outstanding() == 2 and lib.live[e.value][1] >= 1 and lib.copies == copies
        assert s.alloc(0).value and ctx.outstanding() == 3
        assert s.out((0,), np.int8).get().shape == (0,)
        n = s.out_opt(False, (4,), F32)
        assert n.ptr is None and n.get() is None and ctx.outstanding() == 4
    assert ctx.outstanding() == 0


# ------------------------------------------------------------------ 4. pointer residues
def _residue_cases(capi):
    """label -> call(ctx, misalign): one call per helper family on a handful of elements."""
    x = np.arange(60, dtype=F32).reshape(1, 4, 3, 5)
    pri, tgt = np.ones((5, 4), F32), np.ones((3, 5, 4), F32)
    nms = capi.nms_desc(1, 2, 5, 0, 0.1, 4, 0.5, 3)
    dd = capi.deconv_desc(1, 2, 3, 3, 2, 2, 2, stride=(2, 2))
    ymap = np.zeros((1, 14, 2, 2), F32)
    img = np.array([[64, 64]], np.int32)
    return {
        "hard_act": lambda c, m: c.hard_act(capi.HARD_SWISH, x, mode="both", misalign=m),
        "se_scale": lambda c, m: c.se_scale(x, np.ones((1, 4), F32), mode="both", misalign=m),
        "shuffle_channel": lambda c, m: c.shuffle_channel(x, 2, mode="i8", misalign=m),
        "shuffle_unit": lambda c, m: c.shuffle_unit(x, x, 2, mode="both", misalign=m),
        "interp": lambda c, m: c.interp(x, (6, 10), mode="both", misalign=m),
        "arg_max": lambda c, m: c.arg_max(x, 1, misalign=m),
        "interp_argmax": lambda c, m: c.interp_argmax(x, (6, 10), misalign=m),
        "transpose": lambda c, m: c.transpose(x, (0, 2, 3, 1), misalign=m),
        "concat": lambda c, m: c.concat([x, x], 1, misalign=m),
        "concat_calib": lambda c, m: c.concat_calib([x, x], 1, 0.5, misalign=m),
        "split": lambda c, m: c.split(x, 1, num=2, misalign=m),
        "concat_nhwc": lambda c, m: c.concat_nhwc([x, x], misalign=m),
        "box_coder_decode": lambda c, m: c.box_coder_decode(pri, tgt, prior_var=pri, misalign=m),
        "yolo_box": lambda c, m: c.yolo_box(ymap, img, [10, 13, 16, 30], 2, 0.01, 32, misalign=m),
        "yolo_head": lambda c, m: c.yolo_head([ymap, ymap], img, [[10, 13, 16, 30]] * 2, 2, 0.01, [32, 16], misalign=m),
        "multiclass_nms": lambda c, m: c.multiclass_nms(np.zeros((1, 5, 4), F32), np.zeros((1, 2, 5), F32), nms, misalign=m),
        "conv2d_transpose": lambda c, m: c.conv2d_transpose(dd, np.zeros((1, 2, 3, 3), np.int8), np.zeros((2, 2, 2, 2), np.int8),
                                                            np.ones(2, F32), None, capi.OUT_F32, misalign=m),
    }


def residues(capi, monkeypatch):
    """{"helper@misalign": [[entry point, residues of its pointer arguments], ...]}: misalign 0 and 1, conv2d_transpose (bytes)
    4 as well."""
    table = {}
    for label, call in _residue_cases(capi).items():
        for m in (0, 1, 4) if label == "conv2d_transpose" else (0, 1):
            ctx, lib = stub_context(capi, monkeypatch)
            call(ctx, m)
            table["%s@%d" % (label, m)] = [[name, res] for name, res in lib.calls]
    return table


# Recorded by running residues() above, this same stub, against the capi.py of the commit before the helpers moved onto
# DeviceScope (None: a null pointer; a list: the elements of a pointer array).
PARENT_RESIDUES = {
    "hard_act@0": [["plhip_hard_act_f32", [0, 0, 0]]],
    "hard_act@1": [["plhip_hard_act_f32", [4, 4, 1]]],
    "se_scale@0": [["plhip_se_scale_f32", [0, 0, 0, 0]]],
    "se_scale@1": [["plhip_se_scale_f32", [4, 0, 4, 1]]],
    "shuffle_channel@0": [["plhip_shuffle_channel_f32", [0, None, 0]]],
    "shuffle_channel@1": [["plhip_shuffle_channel_f32", [4, None, 1]]],
    "shuffle_unit@0": [["plhip_shuffle_unit_f32", [0, 0, 0, 0, 0]]],
    "shuffle_unit@1": [["plhip_shuffle_unit_f32", [4, 4, 4, 4, 1]]],
    "interp@0": [["plhip_interp_f32", [0, 0, 0]]],
    "interp@1": [["plhip_interp_f32", [4, 4, 1]]],
    "arg_max@0": [["plhip_arg_max_f32", [0, 0]]],
    "arg_max@1": [["plhip_arg_max_f32", [4, 8]]],
    "interp_argmax@0": [["plhip_interp_argmax_f32", [0, 0]]],
    "interp_argmax@1": [["plhip_interp_argmax_f32", [4, 8]]],
    "transpose@0": [["plhip_transpose_f32", [0, 0]]],
    "transpose@1": [["plhip_transpose_f32", [4, 4]]],
    "concat@0": [["plhip_concat_f32", [[0, 0], 0]]],
    "concat@1": [["plhip_concat_f32", [[4, 4], 4]]],
    "concat_calib@0": [["plhip_concat_calib_f32", [[0, 0], 0, 0]]],
    "concat_calib@1": [["plhip_concat_calib_f32", [[4, 4], 4, 1]]],
    "split@0": [["plhip_split_f32", [0, None, [0, 0]]]],
    "split@1": [["plhip_split_f32", [4, None, [4, 4]]]],
    "concat_nhwc@0": [["plhip_concat_nhwc_f32", [[0, 0], 0]]],
    "concat_nhwc@1": [["plhip_concat_nhwc_f32", [[4, 4], 4]]],
    "box_coder_decode@0": [["plhip_box_coder_decode_f32", [0, 0, None, 0, 0]]],
    "box_coder_decode@1": [["plhip_box_coder_decode_f32", [4, 4, None, 4, 4]]],
    "yolo_box@0": [["plhip_yolo_box_f32", [0, 0, 0, 0]]],
    "yolo_box@1": [["plhip_yolo_box_f32", [4, 0, 4, 4]]],
    "yolo_head@0": [["plhip_yolo_head_f32", [[0, 0], 0, 0, 0]]],
    "yolo_head@1": [["plhip_yolo_head_f32", [[4, 4], 0, 4, 4]]],
    "multiclass_nms@0": [["plhip_multiclass_nms_f32", [0, 0, 0, 0, 0, 0]]],
    "multiclass_nms@1": [["plhip_multiclass_nms_f32", [4, 4, 0, 0, 0, 0]]],
    "conv2d_transpose@0": [["plhip_pack_deconv_weights", [0, 0]], ["plhip_conv2d_transpose_int8", [0, 0, 0, None, 0]]],
    "conv2d_transpose@1": [["plhip_pack_deconv_weights", [0, 0]], ["plhip_conv2d_transpose_int8", [0, 0, 0, None, 1]]],
    "conv2d_transpose@4": [["plhip_pack_deconv_weights", [0, 0]], ["plhip_conv2d_transpose_int8", [0, 0, 0, None, 4]]],
}


def test_helpers_keep_every_pointer_residue(pkg, monkeypatch):
    got = residues(pkg.capi, monkeypatch)
    assert sorted(got) == sorted(PARENT_RESIDUES)
    for label in PARENT_RESIDUES:
        assert got[label] == PARENT_RESIDUES[label], label


def test_conv2d_places_x_and_y_and_returns_the_margins(pkg, monkeypatch):
    """Context.conv2d over the stub library, as conv2d_fused (test_tail_cases.py): x lies misalign[0] bytes and y misalign[1]
    elements past a 16-byte boundary, every other operand on one; with a sentinel the allocation comes back filled around the
    tensor, and without either argument the call is what it always was."""
    capi = pkg.capi
    d = capi.conv_desc(1, 16, 4, 4, 8, 1, 1)
    x, w, sc = np.zeros((1, 16, 4, 4), np.int8), np.zeros((8, 16, 1, 1), np.int8), np.ones(8, F32)

    def call(out_kind, **kw):
        ctx, lib = stub_context(capi, monkeypatch)
        r = ctx.conv2d(d, x, w, sc, None, out_kind, **kw)
        assert ctx.outstanding() == 0 and not lib.live
        return r, dict(lib.calls)["plhip_conv2d_int8"]
    # x, packed weights, scale, bias, y, workspace
    r, got = call(capi.OUT_F32)
    assert got == [0, 0, 0, None, 0, 0] and r.shape == (1, 8, 4, 4) and r.dtype == F32
    r, got = call(capi.OUT_F32, misalign=(3, 1), sentinel=0xA5)
    assert got == [3, 0, 0, None, 4, 0]
    y, m = r
    assert y.shape == (1, 8, 4, 4) and y.dtype == F32 and (y.view(np.uint8) == 0xA5).all()
    assert m.dtype == np.uint8 and m.size == 2 * capi.MARGIN_GUARD + 4 + capi.SCOPE_SLACK and (m == 0xA5).all()
    r, got = call(capi.OUT_I8, misalign=(0, 3), sentinel=0x80)
    assert got == [0, 0, 0, None, 3, 0] and r[0].dtype == np.int8 and (r[0] == -128).all() and r[1].size == 2 * capi.MARGIN_GUARD + 3 + capi.SCOPE_SLACK
    r, got = call(capi.OUT_I32, misalign=2)
    assert got == [2, 0, 0, None, 8, 0] and r.dtype == np.int32
    r, got = call(capi.OUT_I8, sentinel=0)
    assert got == [0, 0, 0, None, 0, 0] and (r[1] == 0).all() and r[1].size == 2 * capi.MARGIN_GUARD + capi.SCOPE_SLACK
