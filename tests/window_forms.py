"""The window forms the reference's input types make of a precedence window, the cases the suite runs them at and the
input builder (tests/test_window_forms_cpu.py, tests/test_window_forms_gpu.py, tests/golden/make_golden_window_forms.py).

A FORM is what an (input_type, allow_rot) pair makes of a window of n nodes in D dimensions (pack.py:276-376):

    input_type / allow_rot                         rows    update_rows   R     static rows
    simple/False, rot/False                        n       1             1     1 + D
    rot-old/True                                   n + 1   1             D!    1 + D
    rot-old/False                                  n + 1   1             1     1 + D
    bot/False                                      3n      3             1     1 + D
    bot-rot, use-static, use-pnet /True            3n      3             D!    1 + D
    mul-with/True                                  3n      3             D!    2 + D
    bot/True (the control: every other GPU file)   3n      3             D!    1 + D

The kernels take n, R, rows, update_rows and static_rows as independent run-time values; the other GPU files only ever
hand them R = D!, rows in {n, 3n} and a static row 0 that equals `column mod n`.  Here row 0 of `static` is an independent
random permutation of the node ids per env AND per rotation copy, so the rows update_dynamic clears
(static[b, 0, ptr] + i * n, pack.py:339-374) and the columns update_mask drops ((ptr mod n) + i * n, pack.py:314-321)
are unrelated, and a kernel that took one from the other -- or the id from the wrong 64-column group of a lane -- fails.

No torch.cuda here: the module is imported by CPU tests and by the fixture generator.
"""
import math
from dataclasses import dataclass, replace

import numpy as np

import stream_cases as S

# form name -> (input_type, allow_rot)
FORMS = {
    "simple": ("simple", False),
    "rot1": ("rot", False),
    "rot-old": ("rot-old", True),
    "rot-old1": ("rot-old", False),
    "bot1": ("bot", False),
    "bot-rot": ("bot-rot", True),
    "use-static": ("use-static", True),
    "use-pnet": ("use-pnet", True),
    "mul-with": ("mul-with", True),
    "bot": ("bot", True),                    # the control
}
_ROWS = {"simple": (1, 0, 1), "rot": (1, 0, 1), "rot-old": (1, 1, 1)}       # input_type -> rows = a * n + b, update_rows
SHADOW_PATHS = ("inplace", "noexpand")       # pack.EpisodeStepper forms that need a bit shadow
# the paths of tests/test_window_forms_gpu.py every form runs ('rollout' runs on ROLLOUT_FORMS, 'reward' on the fixture's
# four tours)
PATHS = ("seams", "seams_nonbinary", "mask_stepper", "mask_stepper_nobits", "env_transition", "stepper") + SHADOW_PATHS
ROLLOUT_FORMS = ("rot-old", "simple")


@dataclass(frozen=True)
class Case:
    """One window shape of one form on one container.  Duck-types stream_cases.Case for group_size / fused_kind /
    shadow_ok / launches (which read D, cs, n, B, R, rows, update_rows, nR, W, L, cells, strategy, hard, path, init_mask,
    nsteps)."""
    form: str
    D: int
    cs: tuple
    n: int
    B: int = 64
    strategy: str = "LB_GREEDY"
    own_window: bool = False      # the window IS c2's / c3's / c4's (n, rows, update_rows, nR): the compiled-in kernels are right
    path: str = "stepper"
    init_mask: bool = True
    hard: bool = False

    @property
    def input_type(self):
        return FORMS[self.form][0]

    @property
    def allow_rot(self):
        return FORMS[self.form][1]

    @property
    def R(self):
        return math.factorial(self.D) if self.allow_rot else 1

    @property
    def rows(self):
        a, b, _ = _ROWS.get(self.input_type, (3, 0, 3))
        return a * self.n + b

    @property
    def update_rows(self):
        return _ROWS.get(self.input_type, (3, 0, 3))[2]

    @property
    def static_rows(self):
        return (2 if self.input_type == "mul-with" else 1) + self.D

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
        return self.n if self.n <= 20 else 4

    @property
    def reward(self):
        return "C+P+S-mcs-soft" if self.strategy == "MACS" else "C+P+S-lb-soft"

    @property
    def name(self):
        return "%s-%dd-n%d-%s%s-B%d" % (self.form, self.D, self.n, "macs" if self.strategy == "MACS" else "lbg",
                                        "x".join(str(v) for v in self.cs[:-1]), self.B)

    @property
    def paths(self):
        ok = S.shadow_ok(self)
        out = tuple(p for p in PATHS if ok or p not in SHADOW_PATHS)
        if self.form in ROLLOUT_FORMS and self.strategy == "LB_GREEDY" and self.n <= 12:
            out += ("rollout",)
        return out


def predicted_kind(c):
    """The launcher whose kernel carries a stepper / EnvTransition step of case c: the rule of stream_cases.fused_kind; a
    window on the two-word shadow (rows > 64) leaves the fused kernels for k_mask_step + the placement, and so does the
    fp32-copy step of a container above the lane kernels."""
    fk = S.fused_kind(c)
    if S.shadow_ok(c):
        return fk if c.rows <= 64 else S.MASK_STEP
    return fk if fk in (S.TRANSITION, S.MACS, S.MACS3) else S.MASK_STEP


def check_keys(c, keys):
    """What the launch record of a stepper / EnvTransition episode of case c must say (a set of stream_cases keys (kind, D, G, nc, mode, extra, wt))"""
    kinds = {k[0] for k in keys}
    assert predicted_kind(c) in kinds, "%s: launcher %d not in %s" % (c.name, predicted_kind(c), sorted(keys))
    for kind, D, G, nc, mode, extra, wt in keys:
        if kind not in (S.TRANSITION, S.MACS, S.MACS3):
            continue                                        # the other launchers have no compiled-in window
        if not c.own_window:                                # (FULL exists on a compiled-in window only)
            assert mode & 24 == 0, "%s runs a kernel with a compiled-in window: %r" % (c.name, (kind, D, G, nc, mode, extra, wt))
            assert mode & 64 == 0, "%s runs a FULL kernel: %r" % (c.name, (kind, D, G, nc, mode, extra, wt))
        if kind == S.MACS and c.W == 7:
            assert extra == 0, "%s runs the kernel with c4's width compiled in: %r" % (c.name, (kind, D, G, nc, mode, extra, wt))


LB2, LB3 = (5, 200), (5, 5, 200)
# The smallest shape at which each edge exists.  (rows = 64 never meets a bit shadow on 'rot-old': n = 63 is odd, so
# nR = 63 / 126 / 378 is no multiple of 4 -- that window runs the element-wise kernel; rows = 65 at n = 64 is the one
# with a single row in plane 1 of the two-word shadow.)
_SHAPES = [
    # ---- R = 1
    Case("simple", 2, LB2, 10),          # nR = 10: no shadow; fp32-copy form, element-wise kernel
    Case("simple", 2, LB2, 12),          # nR = 12: shadow, nc = 1
    Case("bot1", 2, LB2, 20),            # nR = 20 and rows = 60 are c2's nR and c4's rows: must run the run-time-shaped kernel
    Case("simple", 2, LB2, 64),          # rows = nR = 64: one full shadow word
    Case("simple", 2, LB2, 68),          # nR = 68 (nc = 2), rows = 68: the two-word shadow, the two-launch step
    Case("rot1", 3, LB3, 16),
    Case("bot1", 2, LB2, 12),
    Case("bot1", 3, LB3, 20),
    Case("rot-old1", 2, LB2, 12),        # rows = 13, nR = 12
    Case("rot-old1", 3, LB3, 64),        # rows = 65 at R = 1 in 3D
    # ---- rot-old
    Case("rot-old", 2, LB2, 10),         # nR = 20, rows = 11: the neighbour of the compiled-in C4S = 5 window
    Case("rot-old", 3, LB3, 10),         # nR = 60, rows = 11: C4S = 15's
    Case("rot-old", 2, LB2, 31),         # rows = 32; nR = 62: no shadow
    Case("rot-old", 2, LB2, 32),         # rows = 33: the n >= 32 guard of the section popcounts
    Case("rot-old", 2, LB2, 63),         # rows = 64; nR = 126: no shadow
    Case("rot-old", 2, LB2, 64),         # rows = 65: plane 1 holds one row; leaves the fused kernels
    Case("rot-old", 2, LB2, 9),          # nR = 18: no shadow
    Case("rot-old", 3, LB3, 8),
    Case("rot-old", 3, LB3, 16),         # nR = 96: two columns per lane, and 64 % n == 0 (the id of a column >= 64)
    Case("rot-old", 3, LB3, 32),         # nR = 192: four columns per lane, rows = 33
    # ---- the other 3n-row forms (12 nodes: no compiled-in window) and the control
    Case("bot-rot", 2, LB2, 12),
    Case("use-static", 3, LB3, 8),
    Case("use-pnet", 2, LB2, 12),
    Case("mul-with", 2, LB2, 12),        # static has 2 + D rows
    Case("mul-with", 3, LB3, 8),
    Case("bot", 2, LB2, 10, own_window=True),
    Case("bot", 2, LB2, 12),
    # ---- placement families: one rot-old and one R = 1 case on each
    Case("rot-old", 2, (7, 200), 20, strategy="MACS"),      # nR = 40, rows = 21: the neighbour of c4's compiled-in window
    Case("simple", 2, (7, 200), 40, strategy="MACS"),       # R = 1 with c4's nR = 40
    Case("bot1", 2, (7, 200), 20, strategy="MACS"),         # R = 1 with c4's n = 20 and rows = 60
    Case("rot-old", 3, LB3, 10, strategy="MACS"),           # MACS 3D 5 x 5: the WL = 5 entries
    Case("rot1", 3, LB3, 16, strategy="MACS"),
    Case("rot-old", 3, (10, 10, 200), 10),                  # k_big_transition
    Case("rot1", 3, (10, 10, 200), 16),
    Case("rot-old", 2, (20, 200), 10, strategy="MACS"),     # k_macs2d_wave_transition
    Case("simple", 2, (20, 200), 12, strategy="MACS"),
    Case("rot-old", 3, (9, 9, 200), 10, strategy="MACS"),   # k_macs3d_wave_transition
    Case("rot1", 3, (9, 9, 200), 16, strategy="MACS"),
]
# every shape on whole workgroups (64 is a multiple of every kernel's envs per workgroup) and ragged (67)
CASES = [replace(c, B=B) for c in _SHAPES for B in (64, 67)]
# c2's own window with 2 + D static rows: the compiled-in kernels are right for it, FULL on the whole batch included, and
# must walk `static` by its 2 + D rows
CASES += [Case("mul-with", 2, LB2, 10, B=B, own_window=True) for B in (64, 67)]
GOLDEN_B = 16
GOLDEN_CASES = [replace(c, B=GOLDEN_B) for c in _SHAPES]

# what the issue names, by (form, D, n[, strategy, sides]) -- tests/test_window_forms_cpu.py checks each against CASES
REQUIRED_SHAPES = [
    ("simple", 2, 10), ("simple", 2, 12), ("bot1", 2, 20), ("simple", 2, 64), ("simple", 2, 68), ("rot1", 3, 16),
    ("rot-old", 2, 10), ("rot-old", 3, 10), ("rot-old", 2, 31), ("rot-old", 2, 32), ("rot-old", 2, 63), ("rot-old", 2, 64),
    ("rot-old", 2, 9),
]
REQUIRED_FAMILIES = [("MACS", (7, 200)), ("MACS", LB3), ("LB_GREEDY", (10, 10, 200)), ("MACS", (20, 200)),
                     ("MACS", (9, 9, 200))]


def density(n):
    """0.1; above 40 nodes 4 / n, so that some columns of the first current_mask stay selectable (0.9 ** 68 of 16 x 68
    columns would leave less than one)."""
    return min(0.1, 4.0 / n)


def build(c, seed, nonbinary=False):
    """-> dict(static (B, static_rows, nR), dynamic (B, rows, nR), tape (B, nsteps) int64), read-only arrays.
    static row 0: an independent random permutation of 0 .. n-1 per env and per rotation copy; sides in 1 .. 4 (every
    block fits every container here); 'mul-with': the target row is random 0 / 1.  dynamic: random 0 / 1, every row
    ('rot-old's extra one included).  tape[t] = node + n * rotation, the nodes a permutation per env.
    ``nonbinary``: a handful of 0.5 / 2.0 entries in dynamic (the re-summing path)."""
    # (the container and the strategy are part of the seed: shapes that share a window do not share their inputs)
    rng = np.random.RandomState(1000 * seed + 7 * c.n + 13 * c.D + c.B + sum(map(ord, c.form + c.strategy)) + 31 * c.cells)
    B, n, R, D = c.B, c.n, c.R, c.D
    static = np.zeros((B, c.static_rows, c.nR), np.float32)
    for b in range(B):
        for r in range(R):
            static[b, 0, r * n:(r + 1) * n] = rng.permutation(n)
    static[:, 1:1 + D] = rng.randint(1, 5, size=(B, D, c.nR))
    if c.input_type == "mul-with":
        static[:, -1] = rng.randint(0, 2, size=(B, c.nR))
    dynamic = (rng.rand(B, c.rows, c.nR) < density(n)).astype(np.float32)
    if nonbinary:
        for v in (0.5, 2.0, 0.5, 2.0, 0.5, 2.0):
            dynamic[rng.randint(B), rng.randint(c.rows), rng.randint(c.nR)] = v
        dynamic[B - 1, c.rows - 1, c.nR - 1] = 0.5
    nodes = np.stack([rng.permutation(n)[:c.nsteps] for _ in range(B)])
    tape = (nodes + n * rng.randint(0, R, size=nodes.shape)).astype(np.int64)
    out = dict(static=static, dynamic=dynamic, tape=tape)
    for a in out.values():
        a.flags.writeable = False
    return out


def oracle_run(O, c, inp, placement=True):
    """The oracle along case c's tape -> dict(initial (B, nR), dynamic / current / mask: one array per step, and with
    ``placement`` the oracle's episode: features, positions, stable, errs, ratio).  Read-only arrays."""
    st, dyn, tape = inp["static"], inp["dynamic"], inp["tape"]
    out = dict(initial=O.initial_mask(dyn, c.n), dynamic=[], current=[], mask=[])
    mask = np.ones((c.B, c.nR), np.float32)
    for t in range(c.nsteps):
        dyn = O.update_dynamic(dyn, st, tape[:, t], c.n, c.update_rows)
        cur, mask = O.update_mask(mask, dyn, tape[:, t], c.n, c.R)
        out["dynamic"].append(dyn); out["current"].append(cur); out["mask"].append(mask)
    if placement:
        blocks = np.stack([st[np.arange(c.B), 1:1 + c.D, tape[:, t]] for t in range(c.nsteps)], axis=1).astype(np.int32)
        out["episode"] = O.run_episodes(O.make_desc(list(c.cs), c.n, c.reward, "diff", c.strategy), blocks)
    for v in out.values():
        for a in (v if isinstance(v, list) else v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.flags.writeable = False
    return out


# ---- the reward tours (pack.reward, pack.py:378-473) ------------------------------------------------------------------
# (form, strategy) of the fixture's four tours; each at n = 8, B = 8, on 2D containers of width 5 and 7 and a 3D one of 5 x 5
TOURS = [("simple", "LB_GREEDY"), ("rot-old", "LB_GREEDY"), ("rot-old", "MACS"), ("mul-with", "MACS")]
TOUR_CONTAINERS = [(2, 5), (2, 7), (3, 5)]                      # (D, container_width)
TOUR_N, TOUR_B, TOUR_H = 8, 8, 64


def tour_case(form, strategy, D, W):
    cs = (W, TOUR_H) if D == 2 else (W, W, TOUR_H)
    return Case(form, D, cs, TOUR_N, B=TOUR_B, strategy=strategy)


def tour_key(form, strategy, D, W):
    return "tour_%s_%s_%dd_w%d" % (form, strategy, D, W)


def tour_inputs(c):
    """-> (static, tour (B, n) int64): the case's static and its whole-episode tape"""
    inp = build(c, seed=5)
    return inp["static"], inp["tape"]
