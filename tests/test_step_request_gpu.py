"""What the fused step's entry points refuse, through the C ABI: the table of tests/step_request_cases.py on
tap_transition / _bits / _first and tap_mask_step_bits / _first, the shapes and alignments the bit shadow refuses, the empty
batch, and the stepper's own refusals.  Every call must return its status before anything is launched: the launch record
(tapenv.h: tap_variant_hits) taken around each group stays empty.  The smallest window with a bit shadow: 2D, W = 5, n = 4
(nR = 8, rows = 12), B = 8.  Every pointer handed in is a live buffer of the full size."""
import ctypes as C

import pytest
import torch

import step_request_cases as R

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
B, W, H = 8, 5, 50


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


@pytest.fixture(scope="module")
def box(T):
    """The context, a container and one live buffer per pointer field (dyn_out with room for a 4-byte offset)."""
    L = T._lib
    env = T.BatchedContainer(B, [W, H], R.N, "C+P+S-lb-soft", "diff", packing_strategy="LB_GREEDY", device=DEV)
    nR = R.N * R.R
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=DEV)
    t = {
        "dyn_in": f32(B, R.ROWS, nR), "dyn_out": f32(B * R.ROWS * nR + 4), "static": f32(B, R.STATIC_ROWS, nR) + 1.0,
        "bits_in": torch.zeros(B, nR, dtype=torch.int64, device=DEV), "bits_out": torch.zeros(B, nR, dtype=torch.int64, device=DEV),
        "ptr": torch.zeros(B, dtype=torch.int64, device=DEV), "mask_in": f32(B, nR) + 1.0, "colsum_in": f32(B, 3, nR),
        "colsum_out": f32(B, 3, nR), "current_out": f32(B, nR), "mask_out": f32(B, nR), "feature_out": torch.zeros(env._feature_shape(), device=DEV),
        "ratio_out": f32(B), "nonbinary_out": torch.zeros(1, dtype=torch.int32, device=DEV),
    }
    buffers = {k: v.data_ptr() for k, v in t.items()}
    buffers["state"] = env._state.data_ptr()
    assert all(v % 16 == 0 for v in buffers.values())
    return dict(L=L, lib=L.lib(), ctx=L.ctx(DEV), stream=L.stream_of(torch.device(DEV)), env=env, tensors=t, buffers=buffers)


def _vp(v):
    return None if v is None else C.c_void_p(v)


def _transition(box, form, desc, p, v, flags):
    """The form's tap_transition* entry with the pointers p (field -> address or None) and the window v."""
    lib, ctx, st = box["lib"], box["ctx"], box["stream"]
    g = lambda f: _vp(p[f])
    head = (ctx, C.byref(desc), g("state"), v["n"], v["R"], v["rows"], v["update_rows"])
    if form == R.COPY:
        return lib.tap_transition(*head, g("dyn_in"), g("static"), v["static_rows"], g("ptr"), g("mask_in"), g("colsum_in"), g("dyn_out"),
                                  g("colsum_out"), g("current_out"), g("mask_out"), g("feature_out"), g("ratio_out"), flags, st)
    if form == R.BITS:
        return lib.tap_transition_bits(*head, g("bits_in"), g("static"), v["static_rows"], g("ptr"), g("mask_in"), g("bits_out"), g("dyn_out"),
                                       g("current_out"), g("mask_out"), g("feature_out"), g("ratio_out"), flags, st)
    return lib.tap_transition_first(*head, g("dyn_in"), g("static"), v["static_rows"], g("ptr"), g("mask_in"), g("bits_out"), g("dyn_out"),
                                    g("current_out"), g("mask_out"), g("feature_out"), g("ratio_out"), g("nonbinary_out"), flags, st)


def _mask_step(box, form, p, v):
    """tap_mask_step_bits / _first with the same arguments."""
    lib, ctx, st = box["lib"], box["ctx"], box["stream"]
    g = lambda f: _vp(p[f])
    head = (ctx, B, v["n"], v["R"], v["rows"], v["update_rows"])
    if form == R.BITS:
        return lib.tap_mask_step_bits(*head, g("bits_in"), g("static"), v["static_rows"], g("ptr"), g("mask_in"), g("bits_out"), g("dyn_out"),
                                      g("current_out"), g("mask_out"), st)
    return lib.tap_mask_step_first(*head, g("dyn_in"), g("static"), v["static_rows"], g("ptr"), g("mask_in"), g("bits_out"), g("dyn_out"),
                                   g("current_out"), g("mask_out"), g("nonbinary_out"), st)


def _nothing_launched(box):
    torch.cuda.synchronize()
    assert box["L"].variant_keys(DEV) == set()


def test_refusal_table_through_the_c_abi(box):
    L, lib, ctx, env = box["L"], box["lib"], box["ctx"], box["env"]
    L.variant_hits_reset(DEV)
    called = 0
    for row in R.ROWS_TABLE:
        if row.from_stepper:
            continue                                        # no public entry point says "from a stepper"
        p, v = R.pointers_of(row, box["buffers"]), R.ints_of(row)
        rc = _transition(box, row.form, env.desc, p, v, row.flags)
        assert rc == row.status, (row.name, rc, lib.tap_last_error(ctx).decode())
        assert lib.tap_last_error(ctx).decode() == row.message, row.name
        called += 1
        if row.mask_step:
            assert _mask_step(box, row.form, p, v) == R.TAP_E_INVALID, row.name
            called += 1
    assert called > 60
    _nothing_launched(box)


def test_shapes_the_bit_shadow_refuses(box):
    """n = 3 (nR = 6: not a multiple of 4) and a dyn_out 4 bytes off its 16-byte alignment: TAP_E_UNSUPPORTED on the bits and
    first forms, fused or stand-alone."""
    L, env = box["L"], box["env"]
    L.variant_hits_reset(DEV)
    valid = lambda form: R.Row("valid", form, R.TAP_OK, "")
    for form in (R.BITS, R.FIRST):
        p = R.pointers_of(valid(form), box["buffers"])
        v = dict(R.ints_of(valid(form)), n=3, rows=9)
        assert _transition(box, form, env.desc, p, v, 0) == R.TAP_E_UNSUPPORTED
        assert _mask_step(box, form, p, v) == R.TAP_E_UNSUPPORTED
        p = dict(p, dyn_out=p["dyn_out"] + 4)
        v = R.ints_of(valid(form))
        assert _transition(box, form, env.desc, p, v, 0) == R.TAP_E_UNSUPPORTED
        assert _mask_step(box, form, p, v) == R.TAP_E_UNSUPPORTED
    _nothing_launched(box)


def test_empty_batch_needs_no_buffers(box):
    L = box["L"]
    desc = L.make_desc(0, [W, H], R.N, "C+P+S-lb-soft", "diff", "LB_GREEDY")
    L.variant_hits_reset(DEV)
    none = {f: None for f in R.POINTERS + ["state"]}
    for form in (R.COPY, R.BITS, R.FIRST):
        assert _transition(box, form, desc, none, R.ints_of(R.Row("valid", form, R.TAP_OK, "")), R.TAP_T_FRESH | R.TAP_T_RATIO) == R.TAP_OK
    _nothing_launched(box)


def test_stepper_refusals(box):
    L, lib, ctx, env, b = box["L"], box["lib"], box["ctx"], box["env"], box["buffers"]
    t = box["tensors"]
    second = {k: torch.zeros_like(t[k]) for k in ("bits_out", "current_out", "mask_out")}

    def buffers(equal_bits):
        buf = L.StepperBuffers()
        buf.bits[0], buf.bits[1] = b["bits_out"], b["bits_out"] if equal_bits else second["bits_out"].data_ptr()
        buf.current[0], buf.current[1] = b["current_out"], second["current_out"].data_ptr()
        buf.mask[0], buf.mask[1] = b["mask_out"], second["mask_out"].data_ptr()
        buf.feature, buf.ratio, buf.nonbinary = b["feature_out"], b["ratio_out"], b["nonbinary_out"]
        return buf

    L.variant_hits_reset(DEV)
    create = lambda buf, h: lib.tap_stepper_create(ctx, C.byref(env.desc), _vp(b["state"]), R.N, R.R, R.ROWS, R.UPDATE_ROWS, R.STATIC_ROWS,
                                                   R.N, C.byref(buf), C.byref(h))
    h = C.c_void_p()
    assert create(buffers(True), h) == R.TAP_E_INVALID and not h.value           # both phases of bits are one buffer
    assert create(buffers(False), h) == R.TAP_OK and h.value
    try:
        assert lib.tap_stepper_step(h, _vp(b["ptr"]), box["stream"]) == R.TAP_E_INVALID
        assert lib.tap_last_error(ctx).decode() == "tap_stepper_begin has not been called"
        assert lib.tap_stepper_steps_done(h) == 0
    finally:
        lib.tap_stepper_destroy(h)
    _nothing_launched(box)
