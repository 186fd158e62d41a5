"""Which precedence-update ("stream wave") kernel instantiations an API-level call launches, restated from the seven
launchers (k_transition, k_transition_macs, k_transition_macs3, k_big_transition, the MACS 2D / 3D wave kernels,
k_mask_step), and the concrete cases the GPU suite runs
(tests/test_stream_variants_gpu.py) with the entries they reach (tests/test_stream_variant_reach_cpu.py).

The facts each launch hands to tap_stream_variant (tap-net_amd/csrc/tap_stream_variant.h) come from these rules:
- tap_write_through (tap_masks.h): write-through when the launch's fp32 tensor, B * rows * nR * 4 bytes, is at
  most TAP_WT_MAX_BYTES = 64 MB (tap_masks.h); mask_finish (tap_masks.h) sets MaskArgs::wt for every launch.
- mask_fast_path_cols (tap_masks.h): on the bit shadow nc = 1 / 2 / 4 for nR <= 64 / 128 / 256; on the fp32
  copy the same when nR % 4 == 0 and nR <= 256 and dyn_out, ptr, static and the column sums are given, else 0.
- tap_group_size (tap_common.h): G = 8 / 16 / 32 / 64 for containers of <= 8 / 16 / 32 / 64 cells; EPB (TransGeom,
  tap_transition.h) = 4 envs per workgroup for G = 64, else 8.
- tap_step_route (tap_step_request.h), TAP_ROUTE_FUSED: LB_GREEDY containers of at most 64 cells (3D: sides <= 8), MACS 2D
  of at most 16 columns and MACS 3D of at most 64 cells (sides <= 8) run the step as ONE k_transition / k_transition_macs /
  k_transition_macs3 launch; the bit-shadow entry points do so for rows <= 64 only, and above that take
  TAP_ROUTE_TWO_LAUNCHES: tap_mask_step_bits / _first (k_mask_step on the two-word shadow) and the placement.
- tap_step_route, TAP_ROUTE_WAVE_*: on the bit shadow with rows <= 64, LB_GREEDY above 64 cells runs
  k_big_transition, MACS 2D above 16 columns k_macs2d_wave_transition, MACS 3D above 64 cells (or a side above 8)
  k_macs3d_wave_transition; their fp32-copy steps (tap_transition) are two launches (k_mask_step + placement).
- transition_macs.hip (tap_transition_macs_launch): the MACS steps stay write-through up to 128 MB per launch.
- the stepper (transition.hip: tap_stepper_create / _begin / _step): a window without a bit shadow
  (tap_step_request.h: tap_window_has_shadow -- nR % 4 != 0, nR > 256 or rows > 128) is carried as the fp32 copy with
  column sums (copy form: begin launches tap_update_mask, k_mask_step on no tensor, then every step is tap_transition's fp32 copy); otherwise begin(initial_mask=True) launches
  tap_mask_step_first with no ptr / static / mask_in, step 0 then reads that shadow and mask (all inputs given),
  and begin(initial_mask=False) makes step 0 build the shadow from fp32 with no mask_in; the in-place form
  (dyn[0] == dyn[1]) sets MaskArgs::inplace from step 1 on.
"""
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass, replace
import itertools

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSITION, MACS, MACS3, BIG, MACS_WAVE, MACS3_WAVE, MASK_STEP = range(7)
WT_MAX_BYTES = 64 << 20
TAP_MACS_M1, TAP_MACS_M2 = 5, 6            # tap_stream_variant.h: the MACS 2D step on the bit shadow (given / built)


@dataclass(frozen=True)
class Case:
    name: str
    D: int
    cs: tuple                 # container sides (W, H) or (W, L, H)
    n: int
    B: int
    input_type: str = "bot"   # 'bot': rows = 3n, three cleared rows; 'rot': rows = n, one
    path: str = "stepper"     # stepper | inplace | noexpand (pack.EpisodeStepper forms) | seam_bits (tap_mask_step_bits) |
                              # seam_transition_bits | seam_transition / seam_mask_step (the C ABI's fp32-copy steps)
    init_mask: bool = True    # stepper: begin(initial_mask=...)
    offset: int = 0           # seams: dyn_out this many bytes into a larger buffer
    episodes: int = 1
    strategy: str = "LB_GREEDY"   # or "MACS"
    hard: bool = False        # LB_GREEDY: C+P+S-lb-hard instead of -soft (k_big_transition's HARD)
    steps: int = 0            # stepper: steps per episode, 0 = n

    @property
    def R(self):
        return math.factorial(self.D)

    @property
    def rows(self):
        return self.n if self.input_type == "rot" else 3 * self.n

    @property
    def update_rows(self):
        return 1 if self.input_type == "rot" else 3

    @property
    def nR(self):
        return self.n * self.R

    @property
    def W(self):
        return self.cs[0]

    @property
    def L(self):
        return self.cs[1] if self.D == 3 else 1

    @property
    def cells(self):
        return self.W * self.L

    @property
    def nsteps(self):
        return self.steps or self.n

    @property
    def reward(self):
        return "C+P+S-mcs-soft" if self.strategy == "MACS" else "C+P+S-lb-hard" if self.hard else "C+P+S-lb-soft"


def group_size(c):
    cells = c.cells
    return 8 if cells <= 8 else 16 if cells <= 16 else 32 if cells <= 32 else 64


def fused_kind(c):
    """The launcher of a one-launch step on this container (None: the step is tap_mask_step* + the placement):
    tap_step_request.h: tap_step_route, tap_is_big / tap_is_big_macs3.  The LDS fits (TapStepCaps: transition.hip's
    transition_caps for the MACS lane kernels, big_transition_pw, macs*_transition_pw) hold for every shape here (small
    heights and n <= 129); tests/test_step_request_cpu.py holds tap_step_route to this model on the host, and the GPU
    file's launch record checks the prediction."""
    if c.strategy == "MACS":
        if c.D == 2:
            return MACS if c.W <= 16 else MACS_WAVE
        return MACS3_WAVE if c.cells > 64 or c.W > 8 or c.L > 8 else MACS3
    big = c.cells > 64 or (c.D == 3 and (c.W > 8 or c.L > 8))
    return BIG if big else TRANSITION


def _wt(c, rows, limit=WT_MAX_BYTES):
    return int(c.B * rows * c.nR * 4 <= limit)


def _cols(nR):
    return 1 if nR <= 64 else 2 if nR <= 128 else 4


def _copy_cols(c):
    return _cols(c.nR) if c.nR % 4 == 0 and c.nR <= 256 else 0


def _facts(c, nc, src, inplace=False, inputs=True, rows=None, update_rows=None, limit=WT_MAX_BYTES):
    rows = c.rows if rows is None else rows
    return dict(nc=nc, src=src, inplace=int(inplace), inputs=int(inputs), wt=_wt(c, rows, limit), n=c.n, rows=rows,
                update_rows=c.update_rows if update_rows is None else update_rows, nR=c.nR)


def shadow_ok(c):
    return c.nR % 4 == 0 and c.nR <= 256 and c.rows <= 128


def launches(c, steps=None):
    """-> [(kind, D, G, facts)] of one episode of case c, in launch order (the launch record's key minus the answer);
    ``steps`` limits the episode (every step after the second repeats the second's facts)."""
    steps = c.nsteps if steps is None else min(steps, c.nsteps)
    fk = fused_kind(c)
    out = []

    def fused(f):
        if fk == TRANSITION:
            G = group_size(c)
            out.append((TRANSITION, c.D, G, dict(f, D=c.D, G=G, EPB=4 if G == 64 else 8, B=c.B, W=0, L=0, hard=0)))
        elif fk in (MACS, MACS3):
            # tap_transition_macs_launch: write-through up to 128 MB; G = 8 / 16 by width (2D), tap_group_size (3D)
            G = (8 if c.W <= 8 else 16) if fk == MACS else group_size(c)
            f = dict(f, wt=_wt(c, f["rows"], 2 * WT_MAX_BYTES))
            out.append((fk, c.D, G, dict(f, D=c.D, G=G, EPB=8, B=c.B, W=c.W, L=c.L, hard=0)))
        else:                                               # wave per container: no D / G in the table
            out.append((fk, 0, 0, dict(f, D=c.D, G=64, EPB=1, B=c.B, W=c.W, L=c.L, hard=int(c.hard and fk == BIG))))

    def mstep(f):
        out.append((MASK_STEP, 0, 0, dict(f, D=0, G=0, EPB=0, B=c.B, W=0, L=0, hard=0)))

    if c.path == "seam_bits":
        mstep(_facts(c, _cols(c.nR), 1))
        return out
    if c.path == "seam_mask_step":
        mstep(_facts(c, _copy_cols(c), 0))
        return out
    single = fk in (TRANSITION, MACS, MACS3)                # the lane-per-cell fused kernels
    if c.path == "seam_transition":                         # tap_transition: the fp32-copy form
        (fused if single else mstep)(_facts(c, _copy_cols(c), 0))
        return out
    if c.path == "seam_transition_bits":
        assert c.rows <= 64
        fused(_facts(c, _cols(c.nR), 1))
        return out
    if not shadow_ok(c):                                    # the stepper's copy form
        mstep(_facts(c, 0, 0, inputs=False, rows=3 * c.n, update_rows=0))   # begin: tap_update_mask
        for _ in range(steps):
            (fused if single else mstep)(_facts(c, _copy_cols(c), 0))
        return out
    one = c.rows <= 64                                      # the fused kernels carry the one-word shadow only
    nc = _cols(c.nR)
    if c.init_mask:
        mstep(_facts(c, nc, 2, inputs=False, update_rows=0))
    for k in range(steps):
        first = k == 0 and not c.init_mask
        f = _facts(c, nc, 2 if first else 1, inplace=(c.path == "inplace" and k > 0), inputs=not first)
        if one:
            fused(f)
        else:
            mstep(dict(f, inplace=0))
    return out


# ---- the host build of the selector (tests/host/stream_variant_host.cpp) -------------------------------------------
_SV = {}


def selector(extra_flags=()):
    key = tuple(extra_flags)
    if key in _SV:
        return _SV[key]
    if shutil.which("g++") is None:
        return None
    so = os.path.join(tempfile.mkdtemp(prefix="sv_"), "libsv.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-fvisibility=hidden", *extra_flags,
                           "-I" + os.path.join(ROOT, "tap-net_amd", "csrc"), os.path.join(ROOT, "tests", "host", "stream_variant_host.cpp"),
                           "-o", so])
    lib = C.CDLL(so)
    lib.sv_select.restype = None
    lib.sv_select.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.sv_table_entry.restype = C.c_int
    lib.sv_table_entry.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.sv_built.restype = C.c_int
    lib.sv_built.argtypes = [C.c_int] * 6
    _SV[key] = lib
    return lib


FACT_COLS = ["nc", "src", "inplace", "inputs", "wt", "n", "rows", "update_rows", "nR", "D", "G", "EPB", "B", "W", "L", "hard"]


def select(lib, kind, facts):
    inp = np.array([[f[k] for k in FACT_COLS] for f in facts], np.int32).reshape(-1, 16)
    out = np.zeros((len(inp), 3), np.int32)
    lib.sv_select(kind, len(inp), inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return [tuple(int(x) for x in r) for r in out]


def keys(lib, launch_list):
    """[(kind, D, G, facts)] -> the set of launch-record keys (kind, D, G, nc, mode, extra, wt)."""
    out = set()
    for kind, D, G, f in launch_list:
        (v,) = select(lib, kind, [f])
        out.add((kind, D, G) + v + (f["wt"],))
    return out


def table(lib, kind):
    out, rows = np.zeros(3, np.int32), []
    while lib.sv_table_entry(kind, len(rows), out.ctypes.data_as(C.c_void_p)):
        rows.append(tuple(int(x) for x in out))
    return rows


# ---- every API-level case of the model ------------------------------------------------------------------------------
# container sides per launcher: LB_GREEDY for each lane group and above 64 cells (k_big_transition), MACS 2D by width (8 /
# 16 lanes, W = 7 for c4's compiled-in width, above 16 columns: the wave kernel), MACS 3D for each lane group (5 x 5 at
# 32 lanes: the compiled-in sides) and above 64 cells (the wave kernel)
SIDES = {
    ("LB_GREEDY", 2): [(5, 1000), (12, 1000), (30, 1000), (50, 1000), (100, 1000)],
    ("LB_GREEDY", 3): [(2, 4, 400), (4, 4, 400), (5, 5, 400), (8, 8, 400), (10, 10, 400)],
    ("MACS", 2): [(5, 1000), (7, 1000), (12, 1000), (20, 1000)],
    ("MACS", 3): [(2, 4, 400), (4, 4, 400), (4, 6, 400), (5, 5, 400), (8, 8, 400), (10, 10, 400)],
}
N_MAX = 129                       # windows of up to 129 nodes: every nR and rows class of each launcher


def batches(c):
    """Whole and ragged workgroups, below and above the write-through limits."""
    per = c.rows * c.nR * 4
    out = [16, 17]
    for lim in (WT_MAX_BYTES, 2 * WT_MAX_BYTES):
        b = -(-(lim + 1) // per)
        out += [b + (-b) % 8, b + (-b) % 8 + 1]
    return out


def all_cases():
    for (strategy, D), sides in SIDES.items():
        for n, it in itertools.product(range(1, N_MAX + 1), ("bot", "rot")):
            for cs in sides:
                for hard in ((False, True) if strategy == "LB_GREEDY" else (False,)):
                    base = Case("x", D, cs, n, 8, it, strategy=strategy, hard=hard)
                    for B in batches(base):
                        for path, init in itertools.product(("stepper", "inplace", "noexpand"), (True, False)):
                            c = replace(base, B=B, path=path, init_mask=init)
                            if not shadow_ok(c) and path != "stepper":
                                continue                  # the copy form has neither form (pack.EpisodeStepper)
                            yield c
                        for path in ("seam_transition", "seam_mask_step"):
                            yield replace(base, B=B, path=path)
                        if shadow_ok(base):
                            yield replace(base, B=B, path="seam_bits", offset=16)
                            if base.rows <= 64:
                                yield replace(base, B=B, path="seam_transition_bits", offset=16)


def reached(lib, cases, steps=None):
    """-> the set of launch-record keys (kind, D, G, nc, mode, extra, wt) the cases launch."""
    by_kind = {}
    for c in cases:
        for kind, D, G, f in launches(c, steps):
            by_kind.setdefault(kind, {})[(D, G) + tuple(f[k] for k in FACT_COLS)] = (D, G, f)
    out = set()
    for kind, d in by_kind.items():
        items = list(d.values())
        for (D, G, f), v in zip(items, select(lib, kind, [f for _, _, f in items])):
            out.add((kind, D, G) + v + (f["wt"],))
    return out


def cost(c):
    """What a case costs the GPU file: elements compared and envs run by the oracle per step, times steps."""
    steps = 1 if c.path.startswith("seam") else (c.steps or c.n) * c.episodes
    return c.B * (c.rows * c.nR + 400) * steps + 50000


# ---- the cases the GPU file runs -------------------------------------------------------------------------------------
# c2's window (n = 10, 2D: nR = 20, rows = 30) and c3's (3D: nR = 60) reach the compiled-in shapes; FULL needs B % EPB == 0
# and all inputs (so begin(initial_mask=True) or a step > 0); 12 nodes run the run-time-shaped kernels; 'rot' windows
# (rows = n) carry up to 64 nodes fused (nR = 2n / 6n: nc = 2 / 4); nR % 4 != 0 (3D 'rot' is always a multiple of 6:
# n odd in 2D) takes the copy form's element-wise path; 65 .. 128 rows the two-word shadow of k_mask_step.  Write-through
# is off above 64 MB per launch: B = 74 000 at c2's window (177.6 MB), 25 000 at c3's (180 MB).
CASES = [
    # 2D, c2's window: FULL (whole batch) / ragged, with and without the initial mask, three stepper forms
    Case("c2-full", 2, (5, 50), 10, 1024),
    Case("c2-ragged-nomask", 2, (5, 50), 10, 1027, init_mask=False),
    Case("c2-inplace-ragged", 2, (5, 50), 10, 1029, path="inplace", episodes=2),
    Case("c2-inplace-full", 2, (5, 50), 10, 1024, path="inplace", init_mask=False),
    Case("c2-noexpand", 2, (5, 50), 10, 1031, path="noexpand"),
    Case("c2-nt-full", 2, (5, 50), 10, 74000),
    Case("c2-nt-inplace-nomask", 2, (5, 50), 10, 74003, path="inplace", init_mask=False),
    Case("c2-nt-ragged", 2, (5, 50), 10, 74001),
    # other lane groups at c2's window
    Case("2d-g16", 2, (12, 40), 10, 515),
    Case("2d-g32", 2, (30, 60), 10, 512, path="inplace", episodes=2),
    Case("2d-g64-nomask", 2, (50, 80), 10, 301, init_mask=False),
    Case("2d-g64-full", 2, (50, 80), 10, 300, path="inplace"),
    # 2D run-time windows: 12 nodes (nc 1), 'rot' 40 nodes (nc 2), odd 'rot' n (nR % 4 != 0: copy form, element-wise)
    Case("2d-n12", 2, (6, 60), 12, 300, path="inplace", episodes=2),
    Case("2d-n12-nomask", 2, (6, 60), 12, 259, init_mask=False),
    Case("2d-rot40", 2, (8, 200), 40, 130, "rot", path="inplace"),
    Case("2d-rot40-nomask", 2, (8, 200), 40, 131, "rot", init_mask=False),
    Case("2d-rot9-copy", 2, (5, 60), 9, 129, "rot"),
    Case("2d-n30-twoword", 2, (5, 150), 30, 100),
    Case("2d-n30-twoword-nomask", 2, (5, 150), 30, 101, init_mask=False),
    Case("2d-n70-copy-nc4", 2, (5, 400), 70, 33),
    # 3D, c3's window
    Case("c3-full", 3, (5, 5, 50), 10, 1024),
    Case("c3-ragged-nomask", 3, (5, 5, 50), 10, 1031, init_mask=False),
    Case("c3-inplace", 3, (5, 5, 50), 10, 1030, path="inplace", episodes=2),
    Case("c3-nt", 3, (5, 5, 50), 10, 25000, path="inplace"),
    Case("c3-nt-inplace-nomask", 3, (5, 5, 50), 10, 25001, path="inplace", init_mask=False),
    Case("c3-nt-ragged", 3, (5, 5, 50), 10, 25003),
    Case("3d-g8", 3, (2, 4, 40), 10, 256),
    Case("3d-g16", 3, (4, 4, 40), 10, 260, path="inplace"),
    Case("3d-g64", 3, (8, 8, 60), 10, 129),
    # 3D run-time windows: 'rot' 20 nodes (nR 120: nc 2), 40 nodes (nR 240: nc 4), 'bot' 8 nodes
    Case("3d-n8", 3, (5, 5, 50), 8, 200, path="inplace", init_mask=False),
    Case("3d-rot20", 3, (5, 5, 80), 20, 130, "rot", path="inplace"),
    Case("3d-rot20-nomask", 3, (5, 5, 80), 20, 131, "rot", init_mask=False),
    Case("3d-rot40", 3, (5, 5, 150), 40, 65, "rot", path="inplace"),
    Case("3d-rot40-nomask", 3, (5, 5, 150), 40, 66, "rot", init_mask=False),
    Case("3d-n22-twoword-nc4", 3, (5, 5, 150), 22, 33),
    # the C ABI with dyn_out 16 / 32 / 48 bytes into a larger buffer: sb_add = 1 / 2 / 3 on write-through launches
    Case("seam-mask-bits-16", 2, (5, 50), 10, 67, path="seam_bits", offset=16),
    Case("seam-mask-bits-32", 2, (5, 50), 10, 67, path="seam_bits", offset=32),
    Case("seam-mask-bits-48", 3, (5, 5, 50), 10, 67, path="seam_bits", offset=48),
    Case("seam-trans-bits-16", 2, (5, 50), 10, 64, path="seam_transition_bits", offset=16),
    Case("seam-trans-bits-32", 3, (5, 5, 50), 10, 67, path="seam_transition_bits", offset=32),
    Case("seam-trans-bits-48", 2, (5, 50), 10, 67, path="seam_transition_bits", offset=48),
    # the rest: the cheapest case (cost() above) of all_cases() for each entry no case above reaches, each entry reachable
    # with write-through stores not yet reached with them, and each (launcher, nc) not yet run with nontemporal stores;
    # two steps each (every later step repeats the second's facts)
    Case("g-lb2-5-n2-rot-seam_mask_step-B16", 2, (5, 1000), 2, 16, input_type="rot", path="seam_mask_step"),
    Case("g-lb2-5-n2-rot-seam_transition-B16", 2, (5, 1000), 2, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-5-n20-bot-stepper-nomask-B6992", 2, (5, 1000), 20, 6992, init_mask=False, steps=2),
    Case("g-lb2-5-n34-rot-seam_transition-B16", 2, (5, 1000), 34, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-5-n34-bot-stepper-B16", 2, (5, 1000), 34, 16, steps=2),
    Case("g-lb2-5-n62-bot-seam_mask_step-B728", 2, (5, 1000), 62, 728, path="seam_mask_step"),
    Case("g-lb2-5-n62-rot-stepper-nomask-B2184", 2, (5, 1000), 62, 2184, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-5-n116-bot-seam_mask_step-B208", 2, (5, 1000), 116, 208, path="seam_mask_step"),
    Case("g-lb2-5-n116-bot-seam_transition-B208", 2, (5, 1000), 116, 208, path="seam_transition"),
    Case("g-lb2-12-n1-rot-stepper-B16", 2, (12, 1000), 1, 16, input_type="rot", steps=1),
    Case("g-lb2-12-n2-rot-inplace-B16", 2, (12, 1000), 2, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb2-12-n2-rot-seam_transition-B16", 2, (12, 1000), 2, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-12-n2-rot-stepper-nomask-B16", 2, (12, 1000), 2, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-12-n10-bot-inplace-B17", 2, (12, 1000), 10, 17, path="inplace", steps=2),
    Case("g-lb2-12-n10-bot-inplace-B16", 2, (12, 1000), 10, 16, path="inplace", steps=2),
    Case("g-lb2-12-n10-bot-seam_transition_bits-B27969", 2, (12, 1000), 10, 27969, path="seam_transition_bits", offset=16),
    Case("g-lb2-12-n10-bot-stepper-nomask-B27968", 2, (12, 1000), 10, 27968, init_mask=False, steps=2),
    Case("g-lb2-12-n10-bot-stepper-nomask-B16", 2, (12, 1000), 10, 16, init_mask=False, steps=2),
    Case("g-lb2-12-n20-bot-stepper-nomask-B6992", 2, (12, 1000), 20, 6992, init_mask=False, steps=2),
    Case("g-lb2-12-n34-rot-inplace-B16", 2, (12, 1000), 34, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb2-12-n34-rot-seam_transition-B16", 2, (12, 1000), 34, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-12-n34-rot-stepper-nomask-B16", 2, (12, 1000), 34, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-12-n62-rot-stepper-nomask-B2184", 2, (12, 1000), 62, 2184, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-12-n66-rot-seam_transition-B16", 2, (12, 1000), 66, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-30-n1-rot-stepper-B16", 2, (30, 1000), 1, 16, input_type="rot", steps=1),
    Case("g-lb2-30-n2-rot-inplace-B16", 2, (30, 1000), 2, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb2-30-n2-rot-seam_transition-B16", 2, (30, 1000), 2, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-30-n2-rot-stepper-nomask-B16", 2, (30, 1000), 2, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-30-n10-bot-inplace-B17", 2, (30, 1000), 10, 17, path="inplace", steps=2),
    Case("g-lb2-30-n10-bot-seam_transition_bits-B27969", 2, (30, 1000), 10, 27969, path="seam_transition_bits", offset=16),
    Case("g-lb2-30-n10-bot-stepper-nomask-B27968", 2, (30, 1000), 10, 27968, init_mask=False, steps=2),
    Case("g-lb2-30-n10-bot-stepper-nomask-B16", 2, (30, 1000), 10, 16, init_mask=False, steps=2),
    Case("g-lb2-30-n20-bot-stepper-nomask-B6992", 2, (30, 1000), 20, 6992, init_mask=False, steps=2),
    Case("g-lb2-30-n34-rot-inplace-B16", 2, (30, 1000), 34, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb2-30-n34-rot-seam_transition-B16", 2, (30, 1000), 34, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-30-n34-rot-stepper-nomask-B16", 2, (30, 1000), 34, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-30-n62-rot-stepper-nomask-B2184", 2, (30, 1000), 62, 2184, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-30-n66-rot-seam_transition-B16", 2, (30, 1000), 66, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-50-n1-rot-stepper-B16", 2, (50, 1000), 1, 16, input_type="rot", steps=1),
    Case("g-lb2-50-n2-rot-inplace-B16", 2, (50, 1000), 2, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb2-50-n2-rot-seam_transition-B16", 2, (50, 1000), 2, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-50-n2-rot-stepper-nomask-B16", 2, (50, 1000), 2, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-50-n10-bot-inplace-B17", 2, (50, 1000), 10, 17, path="inplace", steps=2),
    Case("g-lb2-50-n10-bot-seam_transition_bits-B27969", 2, (50, 1000), 10, 27969, path="seam_transition_bits", offset=16),
    Case("g-lb2-50-n10-bot-stepper-nomask-B27968", 2, (50, 1000), 10, 27968, init_mask=False, steps=2),
    Case("g-lb2-50-n20-bot-stepper-nomask-B6992", 2, (50, 1000), 20, 6992, init_mask=False, steps=2),
    Case("g-lb2-50-n34-rot-inplace-B16", 2, (50, 1000), 34, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb2-50-n34-rot-seam_transition-B16", 2, (50, 1000), 34, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-50-n34-rot-stepper-nomask-B16", 2, (50, 1000), 34, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-50-n62-rot-stepper-nomask-B2184", 2, (50, 1000), 62, 2184, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-50-n66-rot-seam_transition-B16", 2, (50, 1000), 66, 16, input_type="rot", path="seam_transition"),
    Case("g-lb2-100-n2-rot-stepper-nomask-B16", 2, (100, 1000), 2, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb2-100-n2-rot-stepper-nomask-hard-B16", 2, (100, 1000), 2, 16, input_type="rot", init_mask=False, hard=True, steps=2),
    Case("g-lb2-100-n20-bot-seam_transition_bits-B6992", 2, (100, 1000), 20, 6992, path="seam_transition_bits", offset=16),
    Case("g-lb2-100-n62-rot-seam_transition_bits-B2184", 2, (100, 1000), 62, 2184, input_type="rot", path="seam_transition_bits", offset=16),
    Case("g-lb3-2x4-n1-rot-stepper-B16", 3, (2, 4, 400), 1, 16, input_type="rot", steps=1),
    Case("g-lb3-2x4-n2-rot-inplace-B16", 3, (2, 4, 400), 2, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb3-2x4-n2-rot-seam_transition-B16", 3, (2, 4, 400), 2, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-2x4-n2-rot-stepper-nomask-B16", 3, (2, 4, 400), 2, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-2x4-n10-bot-inplace-B17", 3, (2, 4, 400), 10, 17, path="inplace", steps=2),
    Case("g-lb3-2x4-n10-bot-inplace-B16", 3, (2, 4, 400), 10, 16, path="inplace", steps=2),
    Case("g-lb3-2x4-n10-bot-stepper-nomask-B16", 3, (2, 4, 400), 10, 16, init_mask=False, steps=2),
    Case("g-lb3-2x4-n12-rot-inplace-B16", 3, (2, 4, 400), 12, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb3-2x4-n12-rot-seam_bits-B16", 3, (2, 4, 400), 12, 16, input_type="rot", path="seam_bits", offset=16),
    Case("g-lb3-2x4-n12-rot-seam_mask_step-B16", 3, (2, 4, 400), 12, 16, input_type="rot", path="seam_mask_step"),
    Case("g-lb3-2x4-n12-rot-seam_transition-B16", 3, (2, 4, 400), 12, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-2x4-n12-rot-stepper-nomask-B16", 3, (2, 4, 400), 12, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-2x4-n22-rot-inplace-B16", 3, (2, 4, 400), 22, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb3-2x4-n22-rot-seam_bits-B16", 3, (2, 4, 400), 22, 16, input_type="rot", path="seam_bits", offset=16),
    Case("g-lb3-2x4-n22-rot-seam_mask_step-B16", 3, (2, 4, 400), 22, 16, input_type="rot", path="seam_mask_step"),
    Case("g-lb3-2x4-n22-rot-seam_transition-B16", 3, (2, 4, 400), 22, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-2x4-n22-rot-stepper-nomask-B16", 3, (2, 4, 400), 22, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-2x4-n108-bot-seam_mask_step-B80", 3, (2, 4, 400), 108, 80, path="seam_mask_step"),
    Case("g-lb3-2x4-n108-bot-seam_transition-B80", 3, (2, 4, 400), 108, 80, path="seam_transition"),
    Case("g-lb3-4x4-n1-rot-stepper-B16", 3, (4, 4, 400), 1, 16, input_type="rot", steps=1),
    Case("g-lb3-4x4-n2-rot-inplace-B16", 3, (4, 4, 400), 2, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb3-4x4-n2-rot-seam_transition-B16", 3, (4, 4, 400), 2, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-4x4-n2-rot-stepper-nomask-B16", 3, (4, 4, 400), 2, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-4x4-n10-bot-inplace-B16", 3, (4, 4, 400), 10, 16, path="inplace", steps=2),
    Case("g-lb3-4x4-n10-bot-stepper-nomask-B16", 3, (4, 4, 400), 10, 16, init_mask=False, steps=2),
    Case("g-lb3-4x4-n12-rot-inplace-B16", 3, (4, 4, 400), 12, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb3-4x4-n12-rot-seam_transition-B16", 3, (4, 4, 400), 12, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-4x4-n12-rot-stepper-nomask-B16", 3, (4, 4, 400), 12, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-4x4-n22-rot-inplace-B16", 3, (4, 4, 400), 22, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb3-4x4-n22-rot-seam_transition-B16", 3, (4, 4, 400), 22, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-4x4-n22-rot-stepper-nomask-B16", 3, (4, 4, 400), 22, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-5x5-n1-rot-stepper-B16", 3, (5, 5, 400), 1, 16, input_type="rot", steps=1),
    Case("g-lb3-5x5-n2-rot-seam_transition-B16", 3, (5, 5, 400), 2, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-5x5-n2-rot-seam_transition_bits-B16", 3, (5, 5, 400), 2, 16, input_type="rot", path="seam_transition_bits", offset=16),
    Case("g-lb3-5x5-n10-bot-inplace-B16", 3, (5, 5, 400), 10, 16, path="inplace", steps=2),
    Case("g-lb3-5x5-n12-rot-seam_transition-B16", 3, (5, 5, 400), 12, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-5x5-n22-rot-seam_transition-B16", 3, (5, 5, 400), 22, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-8x8-n1-rot-stepper-B16", 3, (8, 8, 400), 1, 16, input_type="rot", steps=1),
    Case("g-lb3-8x8-n2-rot-inplace-B16", 3, (8, 8, 400), 2, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb3-8x8-n2-rot-seam_transition-B16", 3, (8, 8, 400), 2, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-8x8-n2-rot-stepper-nomask-B16", 3, (8, 8, 400), 2, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-8x8-n10-bot-inplace-B17", 3, (8, 8, 400), 10, 17, path="inplace", steps=2),
    Case("g-lb3-8x8-n10-bot-inplace-B16", 3, (8, 8, 400), 10, 16, path="inplace", steps=2),
    Case("g-lb3-8x8-n10-bot-stepper-nomask-B16", 3, (8, 8, 400), 10, 16, init_mask=False, steps=2),
    Case("g-lb3-8x8-n12-rot-inplace-B16", 3, (8, 8, 400), 12, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb3-8x8-n12-rot-seam_transition-B16", 3, (8, 8, 400), 12, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-8x8-n12-rot-stepper-nomask-B16", 3, (8, 8, 400), 12, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-8x8-n22-rot-inplace-B16", 3, (8, 8, 400), 22, 16, input_type="rot", path="inplace", steps=2),
    Case("g-lb3-8x8-n22-rot-seam_transition-B16", 3, (8, 8, 400), 22, 16, input_type="rot", path="seam_transition"),
    Case("g-lb3-8x8-n22-rot-stepper-nomask-B16", 3, (8, 8, 400), 22, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-10x10-n12-rot-stepper-nomask-hard-B16", 3, (10, 10, 400), 12, 16, input_type="rot", init_mask=False, hard=True, steps=2),
    Case("g-lb3-10x10-n12-rot-stepper-nomask-B16", 3, (10, 10, 400), 12, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-10x10-n22-rot-stepper-nomask-B16", 3, (10, 10, 400), 22, 16, input_type="rot", init_mask=False, steps=2),
    Case("g-lb3-10x10-n22-rot-stepper-nomask-hard-B16", 3, (10, 10, 400), 22, 16, input_type="rot", init_mask=False, hard=True, steps=2),
    Case("g-lb3-10x10-n42-rot-seam_transition_bits-B1592", 3, (10, 10, 400), 42, 1592, input_type="rot", path="seam_transition_bits", offset=16),
    Case("g-mac2-5-n1-rot-stepper-B16", 2, (5, 1000), 1, 16, input_type="rot", strategy="MACS", steps=1),
    Case("g-mac2-5-n2-rot-inplace-B16", 2, (5, 1000), 2, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac2-5-n2-rot-seam_transition-B16", 2, (5, 1000), 2, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac2-5-n2-rot-stepper-nomask-B16", 2, (5, 1000), 2, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac2-5-n32-bot-seam_transition-B5464", 2, (5, 1000), 32, 5464, path="seam_transition", strategy="MACS"),
    Case("g-mac2-5-n34-rot-inplace-B16", 2, (5, 1000), 34, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac2-5-n34-rot-seam_transition-B16", 2, (5, 1000), 34, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac2-5-n34-rot-stepper-nomask-B16", 2, (5, 1000), 34, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac2-5-n62-bot-seam_transition-B1456", 2, (5, 1000), 62, 1456, path="seam_transition", strategy="MACS"),
    Case("g-mac2-5-n66-rot-seam_transition-B16", 2, (5, 1000), 66, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac2-5-n115-bot-seam_transition-B424", 2, (5, 1000), 115, 424, path="seam_transition", strategy="MACS"),
    Case("g-mac2-5-n122-bot-seam_transition-B376", 2, (5, 1000), 122, 376, path="seam_transition", strategy="MACS"),
    Case("g-mac2-7-n20-bot-inplace-B16", 2, (7, 1000), 20, 16, path="inplace", strategy="MACS", steps=2),
    Case("g-mac2-7-n20-bot-stepper-nomask-B16", 2, (7, 1000), 20, 16, init_mask=False, strategy="MACS", steps=2),
    Case("g-mac2-12-n1-rot-stepper-B16", 2, (12, 1000), 1, 16, input_type="rot", strategy="MACS", steps=1),
    Case("g-mac2-12-n2-rot-inplace-B16", 2, (12, 1000), 2, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac2-12-n2-rot-seam_transition-B16", 2, (12, 1000), 2, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac2-12-n2-rot-stepper-nomask-B16", 2, (12, 1000), 2, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac2-12-n34-rot-inplace-B16", 2, (12, 1000), 34, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac2-12-n34-rot-seam_transition-B16", 2, (12, 1000), 34, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac2-12-n34-rot-stepper-nomask-B16", 2, (12, 1000), 34, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac2-12-n66-rot-seam_transition-B16", 2, (12, 1000), 66, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac2-20-n2-rot-stepper-nomask-B16", 2, (20, 1000), 2, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac2-20-n20-bot-seam_transition_bits-B6992", 2, (20, 1000), 20, 6992, path="seam_transition_bits", offset=16, strategy="MACS"),
    Case("g-mac2-20-n34-rot-stepper-nomask-B16", 2, (20, 1000), 34, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac2-20-n62-rot-seam_transition_bits-B2184", 2, (20, 1000), 62, 2184, input_type="rot", path="seam_transition_bits", offset=16, strategy="MACS"),
    Case("g-mac3-2x4-n1-rot-stepper-B16", 3, (2, 4, 400), 1, 16, input_type="rot", strategy="MACS", steps=1),
    Case("g-mac3-2x4-n2-rot-inplace-B16", 3, (2, 4, 400), 2, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-2x4-n2-rot-seam_transition-B16", 3, (2, 4, 400), 2, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-2x4-n2-rot-stepper-nomask-B16", 3, (2, 4, 400), 2, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-2x4-n10-bot-seam_transition-B18648", 3, (2, 4, 400), 10, 18648, path="seam_transition", strategy="MACS"),
    Case("g-mac3-2x4-n12-rot-inplace-B16", 3, (2, 4, 400), 12, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-2x4-n12-rot-seam_transition-B16", 3, (2, 4, 400), 12, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-2x4-n12-rot-stepper-nomask-B16", 3, (2, 4, 400), 12, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-2x4-n20-bot-seam_transition-B4664", 3, (2, 4, 400), 20, 4664, path="seam_transition", strategy="MACS"),
    Case("g-mac3-2x4-n22-rot-inplace-B16", 3, (2, 4, 400), 22, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-2x4-n22-rot-seam_transition-B16", 3, (2, 4, 400), 22, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-2x4-n22-rot-stepper-nomask-B16", 3, (2, 4, 400), 22, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-2x4-n40-bot-seam_transition-B1168", 3, (2, 4, 400), 40, 1168, path="seam_transition", strategy="MACS"),
    Case("g-mac3-2x4-n108-bot-seam_transition-B160", 3, (2, 4, 400), 108, 160, path="seam_transition", strategy="MACS"),
    Case("g-mac3-4x4-n1-rot-stepper-B16", 3, (4, 4, 400), 1, 16, input_type="rot", strategy="MACS", steps=1),
    Case("g-mac3-4x4-n2-rot-inplace-B16", 3, (4, 4, 400), 2, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-4x4-n2-rot-seam_transition-B16", 3, (4, 4, 400), 2, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-4x4-n2-rot-stepper-nomask-B16", 3, (4, 4, 400), 2, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-4x4-n12-rot-inplace-B16", 3, (4, 4, 400), 12, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-4x4-n12-rot-seam_transition-B16", 3, (4, 4, 400), 12, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-4x4-n12-rot-stepper-nomask-B16", 3, (4, 4, 400), 12, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-4x4-n22-rot-inplace-B16", 3, (4, 4, 400), 22, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-4x4-n22-rot-seam_transition-B16", 3, (4, 4, 400), 22, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-4x4-n22-rot-stepper-nomask-B16", 3, (4, 4, 400), 22, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-4x6-n1-rot-stepper-B16", 3, (4, 6, 400), 1, 16, input_type="rot", strategy="MACS", steps=1),
    Case("g-mac3-4x6-n2-rot-inplace-B16", 3, (4, 6, 400), 2, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-4x6-n2-rot-seam_transition-B16", 3, (4, 6, 400), 2, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-4x6-n2-rot-stepper-nomask-B16", 3, (4, 6, 400), 2, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-4x6-n12-rot-inplace-B16", 3, (4, 6, 400), 12, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-4x6-n12-rot-seam_transition-B16", 3, (4, 6, 400), 12, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-4x6-n12-rot-stepper-nomask-B16", 3, (4, 6, 400), 12, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-4x6-n22-rot-inplace-B16", 3, (4, 6, 400), 22, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-4x6-n22-rot-seam_transition-B16", 3, (4, 6, 400), 22, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-4x6-n22-rot-stepper-nomask-B16", 3, (4, 6, 400), 22, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-5x5-n1-rot-stepper-B16", 3, (5, 5, 400), 1, 16, input_type="rot", strategy="MACS", steps=1),
    Case("g-mac3-5x5-n2-rot-inplace-B16", 3, (5, 5, 400), 2, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-5x5-n2-rot-seam_transition-B16", 3, (5, 5, 400), 2, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-5x5-n2-rot-stepper-nomask-B16", 3, (5, 5, 400), 2, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-5x5-n12-rot-inplace-B16", 3, (5, 5, 400), 12, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-5x5-n12-rot-seam_transition-B16", 3, (5, 5, 400), 12, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-5x5-n12-rot-stepper-nomask-B16", 3, (5, 5, 400), 12, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-5x5-n22-rot-inplace-B16", 3, (5, 5, 400), 22, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-5x5-n22-rot-seam_transition-B16", 3, (5, 5, 400), 22, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-5x5-n22-rot-stepper-nomask-B16", 3, (5, 5, 400), 22, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-8x8-n1-rot-stepper-B16", 3, (8, 8, 400), 1, 16, input_type="rot", strategy="MACS", steps=1),
    Case("g-mac3-8x8-n2-rot-inplace-B16", 3, (8, 8, 400), 2, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-8x8-n2-rot-seam_transition-B16", 3, (8, 8, 400), 2, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-8x8-n2-rot-stepper-nomask-B16", 3, (8, 8, 400), 2, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-8x8-n12-rot-inplace-B16", 3, (8, 8, 400), 12, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-8x8-n12-rot-seam_transition-B16", 3, (8, 8, 400), 12, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-8x8-n12-rot-stepper-nomask-B16", 3, (8, 8, 400), 12, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-8x8-n22-rot-inplace-B16", 3, (8, 8, 400), 22, 16, input_type="rot", path="inplace", strategy="MACS", steps=2),
    Case("g-mac3-8x8-n22-rot-seam_transition-B16", 3, (8, 8, 400), 22, 16, input_type="rot", path="seam_transition", strategy="MACS"),
    Case("g-mac3-8x8-n22-rot-stepper-nomask-B16", 3, (8, 8, 400), 22, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-10x10-n2-rot-stepper-nomask-B16", 3, (10, 10, 400), 2, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-10x10-n10-bot-seam_transition_bits-B9328", 3, (10, 10, 400), 10, 9328, path="seam_transition_bits", offset=16, strategy="MACS"),
    Case("g-mac3-10x10-n12-rot-stepper-nomask-B16", 3, (10, 10, 400), 12, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-10x10-n20-bot-seam_transition_bits-B2336", 3, (10, 10, 400), 20, 2336, path="seam_transition_bits", offset=16, strategy="MACS"),
    Case("g-mac3-10x10-n22-rot-stepper-nomask-B16", 3, (10, 10, 400), 22, 16, input_type="rot", init_mask=False, strategy="MACS", steps=2),
    Case("g-mac3-10x10-n42-rot-seam_transition_bits-B1592", 3, (10, 10, 400), 42, 1592, input_type="rot", path="seam_transition_bits", offset=16, strategy="MACS"),
]
