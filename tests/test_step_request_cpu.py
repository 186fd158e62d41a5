"""tap-net_amd/csrc/tap_step_request.h compiled with g++ (tests/host/step_request_host.cpp): the route of a fused step
against tests/stream_cases.py's independent model over every case of its generator, each LDS fit switched off in turn, the
shadow predicate on its edges, and the request check against the refusal table of tests/step_request_cases.py.  No GPU
needed; the same table goes through the C ABI in tests/test_step_request_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import step_request_cases as R
import stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED, WAVE_BIG, WAVE_MACS2, WAVE_MACS3, TWO_LAUNCHES = range(5)          # tap_step_request.h: TapStepRoute
ALL_CAPS, WAVE_FROM = 15, 17                                               # every fit holds; tap_macs2d_wave_from()'s default
STRATEGY = {"LB_GREEDY": 0, "MACS": 1, "LB": 2}                            # tapenv.h
# stream_cases' launcher of a one-launch step -> the route that launches it
ROUTE_OF = {S.TRANSITION: FUSED, S.MACS: FUSED, S.MACS3: FUSED, S.BIG: WAVE_BIG, S.MACS_WAVE: WAVE_MACS2, S.MACS3_WAVE: WAVE_MACS3}


@pytest.fixture(scope="module")
def srq(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("srq") / "libsrq.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(ROOT, "tap-net_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "step_request_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.srq_has_shadow.restype = C.c_int
    lib.srq_has_shadow.argtypes = [C.c_int] * 2
    lib.srq_route.restype = C.c_int
    lib.srq_route.argtypes = [C.c_int] * 8
    lib.srq_route_launches.restype = C.c_int
    lib.srq_route_launches.argtypes = [C.c_int]
    lib.srq_check.restype = C.c_int
    lib.srq_check.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    return lib


def _model_steps(c):
    """[(form, model's route)] of the routed steps of case c: the stepper's steps 0 and 1 (its begin launches
    tap_mask_step_first / tap_update_mask directly: no route), or the one step of a tap_transition* seam."""
    fk = S.fused_kind(c)
    single = fk in (S.TRANSITION, S.MACS, S.MACS3)
    one = c.rows <= 64
    copy_route = FUSED if single else TWO_LAUNCHES
    bits_route = ROUTE_OF[fk] if one else TWO_LAUNCHES
    if c.path == "seam_transition":
        return [(R.COPY, copy_route)]
    if c.path == "seam_transition_bits":
        return [(R.BITS, bits_route)]
    if c.path in ("seam_bits", "seam_mask_step"):
        return []                                              # tap_mask_step*: not a fused step
    if not S.shadow_ok(c):
        return [(R.COPY, copy_route)] * min(2, c.nsteps)
    return [(R.BITS if (k > 0 or c.init_mask) else R.FIRST, bits_route) for k in range(min(2, c.nsteps))]


def _route(srq, cache, form, c, caps=ALL_CAPS):
    key = (form, c.rows, c.strategy, c.D, c.W, c.L, caps)
    if key not in cache:
        cache[key] = srq.srq_route(form, c.rows, STRATEGY[c.strategy], c.D, c.W, c.L, caps, WAVE_FROM)
    return cache[key]


def test_route_equals_the_model_for_every_case(srq):
    cache, walked = {}, 0
    for c in S.all_cases():
        assert bool(srq.srq_has_shadow(c.rows, c.nR)) == S.shadow_ok(c), c      # which form the stepper fills
        for form, want in _model_steps(c):
            got = _route(srq, cache, form, c)
            assert got == want, (c, form, got, want)
            walked += 1
    assert walked > 100000 and {r for r in cache.values()} == {FUSED, WAVE_BIG, WAVE_MACS2, WAVE_MACS3, TWO_LAUNCHES}


def test_route_agrees_with_the_launch_list(srq):
    """The model's terms above (fused_kind, single, one, shadow_ok) and its launch list say the same: a routed step's entry in
    stream_cases.launches() is k_mask_step exactly when the route is the two launches."""
    cache = {}
    for c in S.CASES:
        steps = _model_steps(c)
        if not steps:
            continue
        listed = S.launches(c, steps=2)
        listed = listed[len(listed) - len(steps):]              # (a stepper's begin comes first)
        for (form, _), (kind, _, _, _) in zip(steps, listed):
            got = _route(srq, cache, form, c)
            assert (kind == S.MASK_STEP) == (got == TWO_LAUNCHES) and (kind == S.MASK_STEP or ROUTE_OF[kind] == got), (c.name, kind, got)


CAP_OF = {WAVE_BIG: 1, WAVE_MACS2: 2, WAVE_MACS3: 4}


def test_each_fit_switched_off_gives_two_launches(srq):
    cache, seen = {}, set()
    for c in S.all_cases():
        if c.B != 16 or c.hard or c.path not in ("stepper", "seam_transition"):
            continue                                            # (the route reads neither B nor hard; one bits and one copy path)
        for form, want in _model_steps(c)[:1]:
            cap = CAP_OF.get(want, 8 if (want == FUSED and c.strategy == "MACS") else 0)
            if cap:
                assert _route(srq, cache, form, c, ALL_CAPS & ~cap) == TWO_LAUNCHES, (c, form, cap)
                seen.add(cap)
            for other in (1, 2, 4, 8):                          # a fit of another family changes nothing
                if other != cap:
                    assert _route(srq, cache, form, c, ALL_CAPS & ~other) == want, (c, form, other)
            assert srq.srq_route_launches(want) == (2 if want == TWO_LAUNCHES else 1)
    assert seen == {1, 2, 4, 8}
    # MACS 2D below the hand-over width stays off the wave kernel (W = 20 with the hand-over moved to 33)
    assert srq.srq_route(R.BITS, 30, STRATEGY["MACS"], 2, 20, 1, ALL_CAPS, 33) == TWO_LAUNCHES
    # the legacy 'LB' placement has no fused step in any form
    assert {srq.srq_route(f, 30, STRATEGY["LB"], 2, 5, 1, ALL_CAPS, WAVE_FROM) for f in (R.COPY, R.BITS, R.FIRST)} == {TWO_LAUNCHES}


def test_shadow_predicate_edges(srq):
    for rows, want in ((64, True), (65, True), (128, True), (129, False)):
        assert bool(srq.srq_has_shadow(rows, 8)) == want, rows
    for nR, want in ((4, True), (6, False), (256, True), (260, False)):
        assert bool(srq.srq_has_shadow(12, nR)) == want, nR


def test_shadow_predicate_agrees_with_the_library(srq):
    path = os.environ.get("TAP_LIB_PATH") or os.path.join(ROOT, "tap-net_amd", "libtapenv.so")
    if not os.path.exists(path):
        pytest.skip("libtapenv.so is not built")
    try:
        lib = C.CDLL(path)
    except OSError as e:
        pytest.skip("libtapenv.so does not load here: %s" % e)
    lib.tap_bits_words.restype = C.c_int
    lib.tap_bits_words.argtypes = [C.c_int, C.c_int]
    for rows in (1, 12, 64, 65, 128, 129, 200):
        for nR in (1, 4, 6, 8, 64, 128, 252, 254, 256, 260):
            words = lib.tap_bits_words(rows, nR)
            assert (words > 0) == bool(srq.srq_has_shadow(rows, nR)), (rows, nR)
            assert words == (0 if not words else (2 if rows > 64 else 1) * nR)


@pytest.mark.parametrize("row", R.ROWS_TABLE, ids=lambda r: r.name)
def test_refusal_table(srq, row):
    buffers = {f: 0x10000 + 0x1000 * i for i, f in enumerate(R.POINTERS + ["state"])}      # addresses only: never read
    p = R.pointers_of(row, buffers)
    v = R.ints_of(row)
    ints = (C.c_int * 6)(v["n"], v["R"], v["rows"], v["update_rows"], v["static_rows"], row.flags)
    ptrs = (C.c_size_t * 14)(*[p[f] or 0 for f in R.POINTERS])
    msg = C.create_string_buffer(64)
    rc = srq.srq_check(row.form, ints, ptrs, 8, R.D, int(row.from_stepper), int(p["state"] is not None), msg)
    assert (rc, msg.value.decode()) == (row.status, row.message)
    # the same request on an empty batch is not looked at
    assert srq.srq_check(row.form, ints, ptrs, 0, R.D, int(row.from_stepper), 0, msg) == R.TAP_OK


def test_valid_requests_pass(srq):
    buffers = {f: 0x10000 + 0x1000 * i for i, f in enumerate(R.POINTERS + ["state"])}
    for form in (R.COPY, R.BITS, R.FIRST):
        p = R.pointers_of(R.Row("valid", form, R.TAP_OK, ""), buffers)
        ints = (C.c_int * 6)(R.N, R.R, R.ROWS, R.UPDATE_ROWS, R.STATIC_ROWS, R.TAP_T_FRESH | R.TAP_T_RATIO)
        ptrs = (C.c_size_t * 14)(*[p[f] or 0 for f in R.POINTERS])
        msg = C.create_string_buffer(64)
        assert srq.srq_check(form, ints, ptrs, 8, R.D, 0, 1, msg) == R.TAP_OK and msg.value == b""
