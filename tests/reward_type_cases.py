"""The reference's legacy reward names (Container.calc_ratio, tools.py:3919-3935), what each must set in a descriptor, and
the shared inputs they are run on (tests/test_reward_types_cpu.py, tests/test_reward_types_gpu.py,
tests/golden/make_golden_reward_types.py).

A reward name decides three things in every placement kernel: the candidate score (C + P) + S with P / S zeroed unless
the name holds a capital 'P' / 'S' (tools.py:2135/2138), the hard-mode walk (the name ends in 'hard', tools.py:2113) and
the ratio formula.  With P and S off a candidate's score is C alone, most candidates of a step tie, and the reference's
first-come order decides -- which every cross-lane reduction has to reproduce.

No torch.cuda here: the module is imported by CPU tests and by the fixture generator.
"""
import hashlib
from dataclasses import dataclass

import numpy as np

import window_forms as WF

# name -> (hard, use P, use S, ratio mode by its oracle_lib / tapenv.h name)
NAMES = {
    "comp": (0, 0, 0, "R_C"),
    "soft": (0, 0, 0, "R_CxS"),
    "hard": (1, 0, 0, "R_CxS"),
    "pyrm": (0, 0, 0, "R_CP"),
    "pyrm-soft": (0, 0, 0, "R_CPxS"),
    "pyrm-hard": (1, 0, 0, "R_CPxS"),
    "pyrm-soft-sum": (0, 0, 0, "R_CPS"),
    "pyrm-hard-sum": (0, 0, 0, "R_CPS"),        # ends in 'sum', not in 'hard': the soft walk (tools.py:2113)
    "pyrm-soft-SUM": (0, 0, 1, "R_2CPS"),
    "pyrm-hard-SUM": (0, 0, 1, "R_2CPS"),
    "CPS": (0, 1, 1, "R_CxPxS"),
}
ALL = list(NAMES)
# one name per flag class -- (soft, -, -), (hard, -, -), (soft, -, S), (soft, P, S) with a ratio mode of its own -- and
# 'pyrm-hard-SUM', whose 'hard' must NOT start the hard walk
REPRESENTATIVES = ["comp", "hard", "pyrm-soft-SUM", "pyrm-hard-SUM", "CPS"]
# one name per ratio mode; 'C+P-lb-soft' is the /2 form
RATIO_NAMES = ["comp", "soft", "pyrm", "pyrm-soft", "pyrm-soft-sum", "pyrm-soft-SUM", "CPS", "C+P-lb-soft"]
RATIO_MODE = dict({k: v[3] for k, v in NAMES.items()}, **{"C+P-lb-soft": "R_CP_HALF"})
# the names tools.calc_positions_mcs has a formula for (tools.py:3281-3309); under any other, and under every name of
# this table in tools.calc_positions_lb_greedy (tools.py:2442-2446), the reference prints and raises UnboundLocalError
MCS_SCORED = ALL
LBG_SCORED = ["C+P-lb-soft"]
FEATURES = ("diff", "zero", "full")


def twin(name):
    """the reward the rest of the suite runs with the same hard flag: what a placement under ``name`` must differ from"""
    return "C+P+S-lb-hard" if name.endswith("hard") else "C+P+S-lb-soft"


def formula(mode, C, P, S):
    """calc_ratio (tools.py:3919-3964) in float64, in the reference's order of operations"""
    return {"R_C": lambda: C / 3, "R_CxS": lambda: C * S / 3, "R_CP": lambda: (C + P) / 3, "R_CPxS": lambda: (C + P) * S / 3,
            "R_CPS": lambda: (C + P + S) / 3, "R_2CPS": lambda: (2 * C + P + S) / 3, "R_CxPxS": lambda: C * P * S / 3,
            "R_CP_HALF": lambda: (C + P) / 2}[mode]()


@dataclass(frozen=True)
class Shape:
    """One container with its block lists: footprint sides in side[0] .. side[1] (capped to the container's), heights in
    1 .. hmax."""
    strategy: str
    cs: tuple
    n: int
    side: tuple
    hmax: int = 4
    B: int = 67
    what: str = ""

    @property
    def D(self):
        return len(self.cs)

    @property
    def name(self):
        return "%s-%s-n%d" % (self.strategy, "x".join(map(str, self.cs)), self.n)

    def blocks(self, B=None):
        """(B, n, D) int32, regenerated from the shape: the same array for every caller"""
        B = self.B if B is None else B
        rng = np.random.RandomState(sum(self.cs) * 31 + self.n * 7 + len(self.strategy) + self.side[1])
        out = np.empty((B, self.n, self.D), np.int32)
        for k in range(self.D - 1):
            out[:, :, k] = np.minimum(rng.randint(self.side[0], self.side[1] + 1, size=(B, self.n)), self.cs[k])
        out[:, :, -1] = rng.randint(1, self.hmax + 1, size=(B, self.n))
        out.flags.writeable = False
        return out


# every name runs on these: the lane kernels of each strategy, 2D and 3D
BASE = [
    Shape("LB_GREEDY", (5, 50), 10, (1, 4)),
    Shape("LB_GREEDY", (5, 5, 50), 10, (1, 4)),
    Shape("LB", (5, 50), 12, (1, 4)),
    Shape("LB", (5, 5, 50), 10, (1, 4)),
    Shape("MACS", (7, 100), 20, (1, 4)),
    Shape("MACS", (5, 5, 50), 10, (1, 4)),
]
# the representatives run on one shape per kernel family
FAMILIES = [
    Shape("LB_GREEDY", (12, 80), 12, (1, 6), 6, what="16 lanes per container"),
    Shape("LB_GREEDY", (30, 80), 16, (1, 8), 5, what="32 lanes"),
    Shape("LB_GREEDY", (50, 80), 16, (1, 11), 5, what="64 lanes"),
    Shape("LB_GREEDY", (2, 4, 60), 20, (1, 3), 2, what="8 lanes, W != L"),
    Shape("LB_GREEDY", (3, 3, 60), 40, (1, 3), 2, what="16 lanes"),
    Shape("LB_GREEDY", (8, 8, 90), 12, (1, 5), 5, what="64 lanes"),
    Shape("LB_GREEDY", (70, 60), 30, (1, 11), 5, B=65, what="one wave per container"),
    Shape("LB_GREEDY", (10, 10, 60), 15, (1, 6), 4, B=65, what="one wave per container, 3D"),
    Shape("LB_GREEDY", (16, 9, 80), 20, (1, 6), 5, B=65, what="one wave per container, W != L"),
    Shape("LB_GREEDY", (100, 80), 40, (4, 29), 5, B=65, what="one wave per container, two cells per lane"),
    Shape("LB_GREEDY", (4100, 60), 16, (200, 1499), 5, B=65, what="one workgroup per container"),
    Shape("MACS", (20, 60), 12, (1, 6), 4, what="MACS 2D wide form"),
    Shape("MACS", (64, 40), 12, (4, 30), 3, B=65, what="MACS 2D wide form, 64 columns"),
    Shape("MACS", (100, 60), 12, (8, 45), 4, B=65, what="MACS 2D above 64 columns"),
    Shape("MACS", (10, 10, 40), 12, (1, 5), 3, B=65, what="MACS 3D above the lane form"),
]
STEP_SHAPES = BASE + FAMILIES


def step_cases():
    """(shape, name, feature) of the stand-alone steps: all names on BASE, the representatives on FAMILIES; the
    feature rotates so that each of diff / zero / full meets every strategy"""
    out = []
    for i, s in enumerate(STEP_SHAPES):
        for j, name in enumerate(ALL if s in BASE else REPRESENTATIVES):
            out.append((s, name, FEATURES[(i + j) % 3]))
    return out


def run(O, shape, name, feature="diff", blocks=None, **kw):
    """the oracle's episodes of ``shape`` under ``name``"""
    blocks = shape.blocks() if blocks is None else blocks
    return O.run_episodes(O.make_desc(list(shape.cs), blocks.shape[1], name, feature, shape.strategy), blocks, **kw)


# ---- fused steps: a 'bot' window of 12 nodes (no compiled-in window) over one small and one wide shape per strategy ----
@dataclass(frozen=True)
class Fused(WF.Case):
    """window_forms.Case under a reward name, with the footprint sides of a Shape"""
    rname: str = "comp"
    side: tuple = (1, 4)
    hmax: int = 4

    @property
    def reward(self):
        return self.rname

    @property
    def name(self):
        return "%s-%s-%s" % (self.strategy, "x".join(map(str, self.cs)), self.rname)


FUSED_SHAPES = [
    ("LB_GREEDY", (5, 50), (1, 4), 4), ("LB_GREEDY", (5, 5, 50), (1, 4), 4), ("LB_GREEDY", (10, 10, 60), (1, 5), 4),
    ("LB_GREEDY", (70, 60), (5, 30), 4),
    ("MACS", (7, 100), (1, 5), 4), ("MACS", (20, 60), (1, 6), 4), ("MACS", (5, 5, 50), (1, 4), 4),
    ("MACS", (10, 10, 40), (1, 5), 3),
]
FUSED_N, FUSED_B = 12, 67


def fused_case(shape, name):
    strategy, cs, side, hmax = shape
    return Fused("bot", len(cs), cs, FUSED_N, B=FUSED_B, strategy=strategy, hard=name.endswith("hard"), rname=name,
                 side=side, hmax=hmax)


def fused_names():
    return list(dict.fromkeys(REPRESENTATIVES + RATIO_NAMES))


def _with_sides(static, cs, side, hmax, rng):
    """footprint sides in side[0] .. side[1] (capped to the container's) and heights in 1 .. hmax for every column of a
    window_forms.build static tensor (whose columns are independent blocks, rotation copies included)"""
    D = len(cs)
    static = static.copy()
    for k in range(D - 1):
        static[:, 1 + k] = np.minimum(rng.randint(side[0], side[1] + 1, size=static[:, 0].shape), cs[k])
    static[:, D] = rng.randint(1, hmax + 1, size=static[:, 0].shape)
    static.flags.writeable = False
    return static


def fused_build(c, seed=0):
    """window_forms.build with the case's sides: the inputs depend on the shape, not on the name"""
    inp = WF.build(WF.Case("bot", c.D, c.cs, c.n, B=c.B, strategy=c.strategy), seed)
    static = _with_sides(inp["static"], c.cs, c.side, c.hmax, np.random.RandomState(17 + seed + sum(c.cs)))
    return dict(static=static, dynamic=inp["dynamic"], tape=inp["tape"])


def fused_blocks(c, inp):
    st, tape = inp["static"], inp["tape"]
    return np.stack([st[np.arange(c.B), 1:1 + c.D, tape[:, t]] for t in range(c.nsteps)], axis=1).astype(np.int32)


# ---- whole episodes ------------------------------------------------------------------------------------------------------
# (D, W, H, n, B, strategy, footprint sides, largest height): a lane-kernel shape and a wave-episode shape per strategy
EPISODE_SHAPES = [
    (2, 5, 50, 12, 130, "LB_GREEDY", (1, 4), 4), (2, 100, 60, 12, 65, "LB_GREEDY", (8, 45), 4),
    (3, 5, 50, 12, 67, "LB_GREEDY", (1, 4), 4), (3, 10, 40, 12, 65, "LB_GREEDY", (1, 6), 3),
    (2, 7, 100, 20, 130, "MACS", (1, 4), 4), (2, 100, 60, 12, 65, "MUL", (8, 45), 4), (3, 5, 50, 10, 67, "MUL", (1, 4), 4),
    (3, 10, 40, 12, 65, "MACS", (1, 6), 3),
]
# the names the whole-episode tests run: one per ratio mode (all of them soft) and two for the hard kernels
EPISODE_NAMES = RATIO_NAMES + ["hard", "pyrm-hard"]


def episode_id(shape):
    return "%dd-W%d-%s" % (shape[0], shape[1], shape[5])


def episode_inputs(shape):
    """-> (static (B, 1 + D, n * D!), tour (B, n), the blocks in tour order (B, n, D) int32): window_forms.build's 'bot'
    window with the shape's sides, its tape as the tour"""
    D, W, H, n, B, strategy, side, hmax = shape
    cs = (W, H) if D == 2 else (W, W, H)
    c = WF.Case("bot", D, cs, n, B=B, strategy="LB_GREEDY" if strategy == "LB_GREEDY" else "MACS")
    assert c.nsteps == n
    inp = WF.build(c, seed=3)
    static = _with_sides(inp["static"], cs, side, hmax, np.random.RandomState(29 + sum(cs) + n))
    return static, inp["tape"], fused_blocks(c, dict(static=static, tape=inp["tape"]))


# ---- the reference fixture (tests/golden/reward_types.npz) -----------------------------------------------------------------
GOLDEN_B = 3
GOLDEN_TRACES = [
    Shape("LB_GREEDY", (5, 50), 10, (1, 4)), Shape("LB_GREEDY", (5, 5, 50), 10, (1, 4)),
    Shape("LB", (5, 50), 10, (1, 4)), Shape("LB", (5, 5, 50), 10, (1, 4)),
    Shape("MACS", (7, 60), 10, (1, 4)), Shape("MACS", (5, 5, 50), 10, (1, 4)),
    # the wide shapes: the kernels that are not lane-per-cell
    Shape("LB_GREEDY", (70, 60), 12, (1, 11), 5), Shape("LB_GREEDY", (10, 10, 60), 12, (1, 4)),
    Shape("MACS", (20, 60), 12, (1, 6)), Shape("MACS", (70, 60), 12, (1, 11)), Shape("MACS", (10, 10, 40), 10, (1, 5), 3),
]
# block lists of calc_positions_lb_greedy / calc_positions_mcs: (cs, n, sides); n = 0 is the empty list
GOLDEN_LISTS = [((5, 50), 10, (1, 4)), ((5, 5, 50), 8, (1, 4)), ((7, 60), 12, (1, 5)), ((20, 60), 10, (1, 6)), ((5, 50), 0, (1, 4))]
GOLDEN_LIST_B = 3


def golden_list(cs, n, side, k):
    rng = np.random.RandomState(100 + 13 * k + sum(cs) + n)
    out = rng.randint(side[0], side[1] + 1, size=(n, len(cs))).astype(np.int32)
    out[:, -1] = rng.randint(1, 5, size=n)
    return out


def trace_key(shape, name):
    return "%s/%s" % (shape.name, name)


LIST_STATUS = ("ok", "UnboundLocalError", "IndexError")      # the fixture's list_status codes
TRACE_DIGEST = 6                                              # bytes kept of a trace's per-step digests


def digest(*arrays):
    h = hashlib.blake2b(digest_size=8)
    for a, dtype in arrays:
        h.update(np.ascontiguousarray(a, dtype=dtype).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def trace_plan():
    """[(shape, name, feature)]: every name on the first six shapes, the representatives on the wide ones"""
    out = []
    for i, s in enumerate(GOLDEN_TRACES):
        for j, name in enumerate(ALL if i < 6 else REPRESENTATIVES):
            out.append((s, name, FEATURES[(i + j) % 3]))
    return out


def list_plan():
    """[(function, cs, n, sides, k, name)]"""
    out = []
    for fn in ("calc_positions_lb_greedy", "calc_positions_mcs"):
        for cs, n, side in GOLDEN_LISTS:
            for k in range(GOLDEN_LIST_B if n else 1):
                for name in ALL + ["C+P-lb-soft"]:
                    out.append((fn, cs, n, side, k, name))
    return out
