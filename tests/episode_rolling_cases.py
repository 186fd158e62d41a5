"""Which whole-episode (episode.hip) and rolling (rolling.hip) kernel instantiations the API launches, restated from the
host code, and the GPU cases that run them (tests/test_episode_rolling_variants_gpu.py).  The reach test
(tests/test_episode_rolling_reach_cpu.py) checks the restatement against the code objects; the GPU test checks every
case's launch record (tapenv.h: tap_variant_hits, kinds 16 .. 21) against `launches(case)`.

Launch-record keys are (kind, D, G, nc, mode, extra, wt), with the per-kind fields of tapenv.h:
  EPISODE        k_episode<D, G, SOFT>          (16, D, G, SOFT, 0, 0, 0)
  EPISODE_MACS2  k_episode_macs2<G, WIDE>       (17, 2, G, WIDE, 0, 0, 0)
  EPISODE_MACS3  k_episode_macs3<G, WL>         (18, 3, G, WL, 0, 0, 0)
  ROLL_STEP      k_rolling_step<D, G, CH>       (19, D, G, 0, CH, 0, wt);  k_rolling_step_soft: nc = 1
  ROLL_WINDOW    k_rolling_window<D, CH>        (20, D, 0, 0, CH, 0, wt);  _wide<D, NW>: (20, D, 0, 1, NW, 0, wt);
                                                                           _big<D, MW>:  (20, D, 0, 2, 0, MW, wt)
  ROLL_INIT      k_rolling_init<D>              (21, D, 0, 0, 0, 0, 0);    _big<D, MW>:  (21, D, 0, 1, 0, MW, 0)

The rules (citations are episode.hip / rolling.hip / tap_common.h / tap_masks.h at the time of writing):
  episode_dispatch (episode.hip:245-261): tap_is_big (tap_common.h:172: LB_GREEDY above 64 cells or a 3D side above 8)
    goes to big.hip, not recorded here; MACS 3D by tap_group_size (tap_common.h:303: the smallest of 8 / 16 / 32 / 64
    that holds W*L), with G = 32 and W == L == 5 taking k_episode_macs3<32, 5> (episode.hip:224); MACS 2D by width:
    W > 32 -> <64, true>, W > 16 -> <32, true>, W <= 8 -> <8, false>, else <16, false> (episode.hip:257-259);
    LB_GREEDY by TAP_DISPATCH_DG with SOFT = !TAP_F_HARD (episode.hip:76), the flag from a reward type ending in "hard".
    A block list is prefetched EP_PF = 32 steps at a time (episode.hip:18); a k_episode workgroup holds 256 / G
    containers (episode.hip:74).
  rolling_step_impl (rolling.hip:1485): one fused launch for LB_GREEDY on a lane-per-cell container and N <= 64 or
    roll_wide_nw(N, child) == 2 (rolling.hip:1025: 65 <= N <= 128 and child <= 32); otherwise the placement and
    rolling_window_impl.  launch_rolling_step (rolling.hip:1442-1453): CH = -2 (ROLL_CH_WIDE) for N > 64, with the hard
    kernel for either reward; else CH = 10 when roll_fast_ok (rolling.hip:660: child == 10), else 0; k_rolling_step_soft
    for soft rewards.  G = tap_group_size of the TARGET container (rolling.hip:1522); ROLL_EPB = 2 instances per
    workgroup (rolling.hip:1070).
  rolling_window_impl (rolling.hip:1399-1430): roll_wide_nw(N, child) = 2 -> k_rolling_window<D, -2>, 3 or 4 ->
    k_rolling_window_wide<D, NW>; otherwise N > 64 -> k_rolling_window_big<D, MW> with MW = 4 up to 256 blocks, 16 up
    to 1 024, 64 above (rolling.hip:1415-1416); otherwise k_rolling_window<D, 10 if child == 10 else 0>.
  tap_rolling_init (rolling.hip:1338-1352): N > 64 -> k_rolling_init_big<D, MW> (same MW), else k_rolling_init<D>.
  wt (rolling.hip:1388, 1504; tap_masks.h:12, 188-194): write-through when B * 3 * child^2 * R * 4 bytes <= 64 MB,
    R = 2 in 2D, 6 in 3D.
  roll_check (rolling.hip:1316): 1 <= child <= min(N, 64), N <= 4 096.
run_rolling_episode (rolling.py:338-460) initialises the windows (tap_rolling_init), emits the first window
(tap_roller_begin or RollingWindows.next: rolling_window_impl), then per one-step window calls rolling_step_impl
(fused=True: tap_roller_step or tap_rolling_step) or the placement plus RollingWindows.next (fused=False); its last
window runs on the stream-wave kernels, which the stream-variant test covers.
"""
import dataclasses
import itertools

EPISODE, EPISODE_MACS2, EPISODE_MACS3, ROLL_STEP, ROLL_WINDOW, ROLL_INIT = range(16, 22)
KINDS = (EPISODE, EPISODE_MACS2, EPISODE_MACS3, ROLL_STEP, ROLL_WINDOW, ROLL_INIT)
WT_MAX_BYTES = 64 << 20
EP_PF = 32
ROLL_EPB = 2
ROLL_MAX_N = 4096


def group_size(cells):
    return 8 if cells <= 8 else 16 if cells <= 16 else 32 if cells <= 32 else 64 if cells <= 64 else 0


def is_big(D, W, L):
    """tap_is_big for LB_GREEDY / tap_is_big_macs* for MACS: beyond the lane-per-cell kernels."""
    return W * L > 64 or (D == 3 and (W > 8 or L > 8))


def roll_wide_nw(N, child):
    nw = (N + 63) // 64
    return nw if 64 < N <= 256 and child * nw <= 64 else 0


def roll_wt(B, D, child):
    return int(B * 3 * child * child * (2 if D == 2 else 6) * 4 <= WT_MAX_BYTES)


def _mw(N):
    return 4 if N <= 256 else 16 if N <= 1024 else 64


def sides(cs):
    D = len(cs)
    return D, int(cs[0]), int(cs[1]) if D == 3 else 1


def episode_key(cs, strategy, hard):
    D, W, L = sides(cs)
    if is_big(D, W, L):
        return None
    G = group_size(W * L)
    if strategy == "MACS":
        if D == 3:
            return (EPISODE_MACS3, 3, G, 5 if (G == 32 and W == 5 and L == 5) else 0, 0, 0, 0)
        G2 = 64 if W > 32 else 32 if W > 16 else 8 if W <= 8 else 16
        return (EPISODE_MACS2, 2, G2, int(W > 16), 0, 0, 0)
    return (EPISODE, D, G, 0 if hard else 1, 0, 0, 0)


def window_key(B, D, N, child):
    wt = roll_wt(B, D, child)
    nw = roll_wide_nw(N, child)
    if nw == 2:
        return (ROLL_WINDOW, D, 0, 0, -2, 0, wt)
    if nw:
        return (ROLL_WINDOW, D, 0, 1, nw, 0, wt)
    if N > 64:
        return (ROLL_WINDOW, D, 0, 2, 0, _mw(N), wt)
    return (ROLL_WINDOW, D, 0, 0, 10 if child == 10 else 0, 0, wt)


def init_key(D, N):
    return (ROLL_INIT, D, 0, 1, 0, _mw(N), 0) if N > 64 else (ROLL_INIT, D, 0, 0, 0, 0, 0)


def fusable(cs, strategy, N, child):
    D, W, L = sides(cs)
    return strategy == "LB_GREEDY" and not is_big(D, W, L) and (N <= 64 or roll_wide_nw(N, child) == 2)


def step_key(B, cs, strategy, hard, N, child):
    """The key of one rolling_step_impl call: the fused kernel, or the window kernel of its two-launch form."""
    D, W, L = sides(cs)
    if not fusable(cs, strategy, N, child):
        return window_key(B, D, N, child)
    ch = -2 if N > 64 else 10 if child == 10 else 0
    return (ROLL_STEP, D, group_size(W * L), int(not hard and N <= 64), ch, 0, roll_wt(B, D, child))


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    entry: str                  # reward | scores | pack_blocks | rolling | rolling_unfused | raw_step
    cs: tuple                   # target container (rolling: (w, H) or (w, w, H))
    B: int
    n: int                      # blocks per episode / instance (rolling: N)
    reward: str = "C+P+S-lb-soft"
    strategy: str = "LB_GREEDY"
    target: int = None          # scores: None, 0 or 1
    child: int = 10
    init: tuple = None          # rolling: initial container of the generator
    sample: int = 0             # rolling: oracle-check every instance (0) or this many, the last one included
    grid: bool = False          # rolling: unit blocks on a grid instead of generated instances
    overflow: bool = False      # episodes: blocks wider / taller than the container

    @property
    def D(self):
        return len(self.cs)

    @property
    def hard(self):
        return self.reward.endswith("hard")


def launches(c):
    """The launch record a case leaves on kinds 16 .. 21."""
    if c.entry in ("reward", "scores", "pack_blocks"):
        k = episode_key(c.cs, c.strategy, c.hard)
        return set() if k is None else {k}
    D, N = c.D, c.n
    if c.entry == "raw_step":
        return {step_key(c.B, c.cs, c.strategy, c.hard, N, c.child)}
    keys = {init_key(D, N), window_key(c.B, D, N, c.child)}
    if c.entry == "rolling" and N > c.child:
        keys.add(step_key(c.B, c.cs, c.strategy, c.hard, N, c.child))
    return keys


# ---- every API-level case, for reachability ---------------------------------------------------------------------------
def _containers():
    for W in range(1, 66):
        yield (W, 200)
    for W in range(1, 10):
        for L in range(1, 10):
            yield (W, L, 200)


def all_cases():
    """A product of the facts the rules read: container, strategy, reward, N, child, batch (small, above 64 MB)."""
    out = []
    for cs in _containers():
        for strategy, reward in (("LB_GREEDY", "C+P+S-lb-soft"), ("LB_GREEDY", "C+P+S-lb-hard"), ("MACS", "C+P+S-mcs-soft")):
            out.append(Case("all", "scores", cs, 1, 10, reward, strategy))
    Ns = (1, 10, 11, 64, 65, 100, 128, 129, 192, 193, 256, 257, 1024, 1025, 4096)
    for cs in ((8, 50), (16, 50), (32, 50), (64, 50), (2, 2, 50), (4, 4, 50), (5, 5, 50), (8, 8, 50), (9, 50)):
        for reward, N, B in itertools.product(("C+P+S-lb-soft", "C+P+S-lb-hard"), Ns, (1, 40000)):
            for child in range(1, min(N, 64) + 1):
                for entry in ("rolling", "rolling_unfused"):
                    out.append(Case("all", entry, cs, B, N, reward, child=child))
    return out


def reached(cases):
    return set().union(*(launches(c) for c in cases))


# ---- the GPU cases ----------------------------------------------------------------------------------------------------
def _ep(name, entry, cs, B, n, reward="C+P+S-lb-soft", strategy="LB_GREEDY", **kw):
    return Case(name, entry, tuple(cs), B, n, reward, strategy, **kw)


def _episode_cases():
    out = []
    # every G, soft and hard, through pack.reward (its 3D container is square, pack.py:408-411) and through
    # pack.episode_scores with W != L; B = 2 workgroups + 1
    for D, shapes in ((2, ((5, 40), (12, 40), (30, 40), (64, 40))), (3, ((2, 2, 40), (4, 4, 40), (5, 5, 40), (8, 8, 40)))):
        for cs in shapes:
            G = group_size(cs[0] * (cs[1] if D == 3 else 1))
            for reward in ("C+P+S-lb-soft", "C+P+S-lb-hard"):
                out.append(_ep("reward-%dd-%s-%s" % (D, "x".join(map(str, cs[:-1])), reward[-4:]), "reward", cs,
                               2 * (256 // G) + 1, 10, reward))
    for cs in ((2, 4, 40), (3, 5, 40), (4, 7, 40), (8, 7, 40)):
        for reward in ("C+P+S-lb-soft", "C+P+S-lb-hard"):
            out.append(_ep("scores-3d-%dx%d-%s" % (cs[0], cs[1], reward[-4:]), "scores", cs,
                           2 * (256 // group_size(cs[0] * cs[1])) + 1, 10, reward))
    # n around the block-list prefetch, B = 1 and B = 1 workgroup + 1
    for n in (1, 31, 32, 33, 65):
        out.append(_ep("scores-2d-n%d" % n, "scores", (6, 4 * n + 10), 1 if n % 2 else 33, n, "C+P+S-lb-hard"))
        out.append(_ep("scores-3d-n%d" % n, "scores", (3, 5, 4 * n + 10), 17, n, "C+P+S-lb-soft"))
        out.append(_ep("macs3-n%d" % n, "scores", (4, 6, 4 * n + 10), 9, n, "C+P+S-mcs-soft", "MACS"))
    # targets of the two-container input types
    for t in (None, 0, 1):
        out.append(_ep("scores-target-%s" % t, "scores", (5, 5, 60), 21, 12, "C+P+S-lb-soft", target=t))
        out.append(_ep("macs2-target-%s" % t, "scores", (10, 60), 21, 12, "C+P+S-mcs-hard", "MACS", target=t))
    # every MACS width class and every MACS 3D lane group (blocks within the container sides)
    for W in (1, 8, 9, 16, 17, 32, 33, 64):
        out.append(_ep("macs2-W%d" % W, "scores", (W, 60), 19, 14, "C+P+S-mcs-soft", "MACS"))
    for cs in ((2, 4, 60), (1, 1, 60), (3, 3, 60), (4, 6, 60), (5, 5, 60), (5, 6, 60), (8, 8, 60), (7, 9 - 1, 60)):
        out.append(_ep("macs3-%dx%d" % cs[:2], "scores", cs, 19, 14, "C+P+S-mcs-hard", "MACS"))
    # explicit block lists (generate.pack_blocks), hard and soft
    for cs in ((7, 50), (3, 3, 50), (8, 8, 50), (2, 2, 50), (20, 50)):
        for reward in ("C+P+S-lb-hard", "C+P+S-lb-soft"):
            out.append(_ep("pack-%s-%s" % ("x".join(map(str, cs[:-1])), reward[-4:]), "pack_blocks", cs, 33, 20, reward))
    # overflow: containers too low, LB_GREEDY and MACS 2D blocks wider than the container, MACS 3D too low
    out += [_ep("overflow-lbg-2d", "scores", (4, 9), 65, 20, "C+P+S-lb-soft", overflow=True),
            _ep("overflow-lbg-3d", "scores", (3, 4, 6), 65, 20, "C+P+S-lb-hard", overflow=True),
            _ep("overflow-reward-3d", "reward", (3, 3, 7), 33, 20, "C+P+S-lb-soft", overflow=True),
            _ep("overflow-pack-2d", "pack_blocks", (3, 12), 33, 20, "C+P+S-lb-hard", overflow=True),
            _ep("overflow-macs2", "scores", (3, 10), 33, 20, "C+P+S-mcs-soft", "MACS", overflow=True),
            _ep("overflow-macs2-wide", "scores", (20, 12), 33, 40, "C+P+S-mcs-hard", "MACS", overflow=True),
            _ep("overflow-macs3", "scores", (4, 4, 5), 33, 20, "C+P+S-mcs-soft", "MACS", overflow=True)]
    return out


def _roll(name, entry, cw, D, N, child, B, reward="C+P+S-lb-soft", init=None, **kw):
    # heights: at most 4 000 (env.hip: the 32-bit sort key); unit blocks on a grid need far less
    H = 2 * N // cw ** (D - 1) + 20 if kw.get("grid") else min(4 * N + 10, 4000)
    cs = (cw, H) if D == 2 else (cw, cw, H)
    iw = init if init is not None else min(cw, 7)
    ih = max(H, 60)
    return Case(name, entry, cs, B, N, reward, child=child, init=(iw, ih) if D == 2 else (iw, iw, ih), **kw)


def _rolling_cases():
    out = []
    # every G in both D (3D: sides 2, 3, 5, 8 -> 4, 9, 25, 64 cells), soft and hard, child 10 and not, odd B
    for D, widths in ((2, (5, 12, 20, 40)), (3, (2, 3, 5, 8))):
        for cw in widths:
            for reward in ("C+P+S-lb-soft", "C+P+S-lb-hard"):
                for child in (10, 7):
                    out.append(_roll("roll-%dd-w%d-%s-c%d" % (D, cw, reward[-4:], child), "rolling", cw, D, 24, child,
                                     2 * ROLL_EPB + 1 if child == 10 else 7, reward))
    # 65 <= N <= 128 with two words per lane (fused, CH = -2), and the shapes it does not fuse
    for D in (2, 3):
        out.append(_roll("roll-%dd-N100-soft" % D, "rolling", 5, D, 100, 12, 5))
        out.append(_roll("roll-%dd-N128-hard" % D, "rolling", 3, D, 128, 32, 3, "C+P+S-lb-hard"))
        out.append(_roll("roll-%dd-N70-c40" % D, "rolling", 5, D, 70, 40, 3))          # window_big<D, 4>
        out.append(_roll("roll-%dd-N150" % D, "rolling", 5, D, 150, 20, 3))           # window_wide<D, 3>
        out.append(_roll("roll-%dd-N200" % D, "rolling", 5, D, 200, 16, 3))           # window_wide<D, 4>
        out.append(_roll("roll-%dd-N300" % D, "rolling", 5, D, 300, 60, 2, grid=True))   # big<D, 16>
        out.append(_roll("roll-%dd-N1025" % D, "rolling", 5, D, 1025, 64, 1, grid=True))  # big<D, 64>
    for D, widths in ((2, (12, 20, 40)), (3, (2, 8))):
        for i, cw in enumerate(widths):
            out.append(_roll("roll-%dd-w%d-N80" % (D, cw), "rolling", cw, D, 80, 16, 3, ("C+P+S-lb-soft", "C+P+S-lb-hard")[i % 2],
                             grid=cw < 3))       # (random blocks on a 2 x 2 base are never all stable: unit blocks)
    # the unfused path over whole batches, every window form
    for D in (2, 3):
        for N, child in ((24, 10), (24, 7), (100, 12)):
            out.append(_roll("unfused-%dd-N%d-c%d" % (D, N, child), "rolling_unfused", 5, D, N, child, 5))
    # initial containers wider than the target: error flags against O.Env.add_new_block's return code
    out.append(_roll("roll-2d-init-wider", "rolling", 3, 2, 24, 10, 9, init=6))
    out.append(_roll("roll-3d-init-wider", "rolling", 2, 3, 20, 10, 9, init=4, reward="C+P+S-lb-hard"))
    # above the 64 MB write-through limit: 3D child 10 at B > 9 320, 2D child 16 at B > 10 922
    out.append(_roll("roll-3d-wt0", "rolling", 5, 3, 12, 10, 9321, sample=16))
    out.append(_roll("roll-2d-wt0", "rolling", 5, 2, 18, 16, 10923, sample=16, reward="C+P+S-lb-hard"))
    # one raw tap_rolling_step into guarded buffers, odd B
    out.append(_roll("raw-3d-step", "raw_step", 5, 3, 20, 10, 7))
    out.append(_roll("raw-2d-step-N100", "raw_step", 8, 2, 100, 12, 5, reward="C+P+S-lb-hard"))
    return out


CASES = _episode_cases() + _rolling_cases()
