"""Which instantiation of a precedence-update ("stream wave") kernel a launch runs: tap-net_amd/csrc/tap_stream_variant.h
(tap_stream_variant and the launchers' tables) compiled for the HOST and checked against the rules restated below, over the
full product of the facts it reads, for every launcher and for the A/B builds that change the rules.  The restatement was
written from the launchers' own selection code before it moved into the header: FULL and INPLACE compile guards out of
the kernels, so a wrong answer here reads through null pointers or past B on the GPU.  No GPU needed."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRANSITION, MACS, MACS3, BIG, MACS_WAVE, MACS3_WAVE, MASK_STEP = range(7)
KINDS = 7
MERGED, C4_5, C4_15, C4_10, INPLACE, FULL = 4, 8, 16, 24, 32, 64

# instantiations per launcher: the .kd symbols of each unit's gfx950 code object (k_transition over D in {2, 3} and
# G in {8, 16, 32, 64}; k_transition_macs over G in {8, 16}; k_transition_macs3 over G in {8, 16, 32, 64})
BUILT = {TRANSITION: 180, MACS: 29, MACS3: 65, BIG: 12, MACS_WAVE: 6, MACS3_WAVE: 6, MASK_STEP: 16}
DG = {TRANSITION: [(D, G) for D in (2, 3) for G in (8, 16, 32, 64)], MACS: [(2, 8), (2, 16)],
      MACS3: [(3, G) for G in (8, 16, 32, 64)], BIG: [(0, 0)], MACS_WAVE: [(0, 0)], MACS3_WAVE: [(0, 0)], MASK_STEP: [(0, 0)]}

BUILDS = {"default": [], "no_full": ["-DTAP_NO_FULL"], "macs_nomerge": ["-DTAP_MACS_NOMERGE"],
          "macs_merge_all": ["-DTAP_MACS_MERGE_ALL"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def sv(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("sv") / "libsv.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-fvisibility=hidden"] + BUILDS[request.param] +
                          ["-I" + os.path.join(ROOT, "tap-net_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "stream_variant_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.sv_select.restype = None
    lib.sv_select.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.sv_table_entry.restype = C.c_int
    lib.sv_table_entry.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.sv_built.restype = C.c_int
    lib.sv_built.argtypes = [C.c_int] * 6
    return request.param, lib


def _table(lib, kind):
    out, rows = np.zeros(3, np.int32), []
    while lib.sv_table_entry(kind, len(rows), out.ctypes.data_as(C.c_void_p)):
        rows.append(tuple(int(x) for x in out))
    return rows


# (n, rows, update_rows, nR): c2's, c3's and c4's windows, a near miss of each, and a window above 64 rows
SHAPES = [(10, 30, 3, 20), (10, 30, 4, 20), (10, 30, 3, 60), (10, 31, 3, 60), (20, 60, 3, 40), (19, 60, 3, 40),
          (10, 100, 3, 20)]
SIDES = [(7, 7), (5, 5), (5, 6), (6, 6)]          # W = 7 (c4), 5 x 5 (c6), near miss, other


def _facts():
    """The product of every fact a launcher's choice reads, as named columns (MaskArgs fields before tap_mask_facts)."""
    cols = ["D", "G", "nc", "src", "inplace", "dyn_out", "shape", "ptr", "static", "mask_in", "ragged", "wt", "sides", "hard"]
    grid = itertools.product((2, 3), (8, 16, 32, 64), (0, 1, 2, 4), (0, 1, 2), (0, 1), (0, 1), range(len(SHAPES)), (0, 1),
                             (0, 1), (0, 1), (0, 1), (0, 1), range(len(SIDES)), (0, 1))
    a = np.array(list(grid), np.int32)
    f = {c: a[:, i] for i, c in enumerate(cols)}
    sh, sd = np.array(SHAPES, np.int32)[f["shape"]], np.array(SIDES, np.int32)[f["sides"]]
    f["n"], f["rows"], f["update_rows"], f["nR"] = sh.T
    f["W"], f["L"] = sd.T
    f["EPB"] = np.where(f["G"] == 64, 4, 8)
    f["B"] = 128 * f["EPB"] + f["ragged"] * 3
    return f


def _select(lib, kind, f):
    cols = [f["nc"], f["src"], f["inplace"] & f["dyn_out"], f["ptr"] & f["static"] & f["mask_in"], f["wt"], f["n"], f["rows"],
            f["update_rows"], f["nR"], f["D"], f["G"], f["EPB"], f["B"], f["W"], f["L"], f["hard"]]
    inp = np.ascontiguousarray(np.stack(cols, axis=1), np.int32)
    out = np.zeros((len(inp), 3), np.int32)
    lib.sv_select(kind, len(inp), inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def _expected(build, kind, f):
    """The launchers' rules, restated (the macro ladders of transition.hip, transition_macs.hip, big.hip, macs_big.hip,
    macs3_big.hip and masks.hip as they stood)."""
    nc, src, D, G = f["nc"], f["src"], f["D"], f["G"]
    fast = (nc == 1) | (nc == 2) | (nc == 4)
    zero = np.zeros_like(nc)
    if kind in (BIG, MACS_WAVE, MACS3_WAVE):
        # switch (mask_fast_path_cols) { case 1, case 2, default: 4 } x (bits_in ? 1 : 2) [x hard]
        return np.stack([np.where((nc == 1) | (nc == 2), nc, 4), np.where(src == 1, 1, 2),
                         f["hard"] if kind == BIG else zero], axis=1)
    if kind == MASK_STEP:
        # mode = (bits_in ? 1 : builds ? 2 : 0) + (wide ? 2 : 0), wide = shadow && rows > 64; default: <0, 0>
        wide = (src != 0) & (f["rows"] > 64)
        return np.stack([np.where(fast, nc, 0), np.where(fast, src + 2 * wide, 0), zero], axis=1)
    inpl = (src == 1) & (f["inplace"] == 1) & (f["dyn_out"] == 1)
    if kind == TRANSITION:
        merged = (D == 2) & (f["wt"] == 1)
        M = np.where(inpl, 1 | INPLACE, np.where(src == 1, np.where(merged, 5, 1), np.where(src == 2, np.where(merged, 6, 2), 0)))
        shaped = (f["n"] == 10) & (f["rows"] == 30) & (f["update_rows"] == 3) & (f["nR"] == np.where(D == 2, 20, 60))
        full = (src == 1) & (f["ptr"] == 1) & (f["static"] == 1) & (f["mask_in"] == 1) & (f["B"] % f["EPB"] == 0)
        if build == "no_full":
            full = np.zeros_like(full)
        shape_bit = np.where(D == 2, C4_5, C4_15)
        on1 = (nc == 1) & ((M & 3) == 1) & shaped
        on2 = (nc == 1) & ((M & 3) == 2) & shaped
        M = np.where(on1, M | shape_bit | np.where(full, FULL, 0), np.where(on2, M | shape_bit, M))
        return np.stack([np.where(fast, nc, 0), np.where(fast, M, 0), zero], axis=1)
    m1, m2 = {"default": (5, 6, 1, 2), "no_full": (5, 6, 1, 2), "macs_nomerge": (1, 2, 1, 2),
              "macs_merge_all": (5, 6, 5, 6)}[build][(0 if kind == MACS else 2):][:2]
    M = np.where(inpl, 1 | INPLACE, np.where(src == 1, m1, np.where(src == 2, m2, 0)))
    if kind == MACS3:
        wl = np.where((G == 32) & (f["W"] == 5) & (f["L"] == 5), 5, 0)                  # also on the element-wise path
        return np.stack([np.where(fast, nc, 0), np.where(fast, M, 0), wl], axis=1)
    c4 = (G == 8) & (nc == 1) & ((M & 3) != 0) & (f["W"] == 7) & (f["n"] == 20) & (f["rows"] == 60) & \
        (f["update_rows"] == 3) & (f["nR"] == 40)
    return np.stack([np.where(fast, nc, 0), np.where(fast, np.where(c4, M | C4_10, M), 0), np.where(fast & c4, 7, 0)], axis=1)


@pytest.fixture(scope="module")
def facts():
    return _facts()


@pytest.mark.parametrize("kind", range(KINDS))
def test_selector_matches_the_rules(sv, facts, kind):
    build, lib = sv
    f = facts
    if kind == MACS:            # MACS 2D runs D = 2 with G = 8 / 16 only, MACS 3D D = 3: restrict to what reaches them
        keep = (f["D"] == 2) & (f["G"] <= 16)
    elif kind == MACS3:
        keep = f["D"] == 3
    else:
        keep = np.ones_like(f["D"], bool)
    f = {k: v[keep] for k, v in f.items()}
    got, want = _select(lib, kind, f), _expected(build, kind, f)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, {k: int(v[bad[0]]) for k, v in f.items()} | {"got": got[bad[0]].tolist(), "want": want[bad[0]].tolist()}

    # every answer is an entry of the launcher's table that is instantiated for its (D, G)
    table = set(_table(lib, kind))
    for (D, G) in DG[kind]:
        sel = np.ones(len(got), bool) if (D, G) == (0, 0) else (f["D"] == D) & (f["G"] == G)
        for v in {tuple(int(x) for x in r) for r in got[sel]}:
            assert v in table, (kind, D, G, v)
            assert lib.sv_built(kind, D, G, *v), (kind, D, G, v)


@pytest.mark.parametrize("kind", range(KINDS))
def test_tables(sv, kind):
    _, lib = sv
    table = _table(lib, kind)
    assert len(set(table)) == len(table)
    n = sum(lib.sv_built(kind, D, G, *v) for (D, G) in DG[kind] for v in table)
    assert n == BUILT[kind]
