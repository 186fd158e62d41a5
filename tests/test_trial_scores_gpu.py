"""Trial placements on the MI355X (trial.hip: k_trial_scores) and the greedy best-ratio orders on top of them.

Scores are compared BIT FOR BIT with the oracle replay of tests/best_order_cases.py (a fresh oracle container takes the
committed blocks plus the candidate, fp64 calc_ratio, -1.0 when the candidate's step raises) and with the stepped form
(``trial_scores(stepped=True)``: nR committed steps on a scratch copy of the blob, kernels the package already had);
``best`` against numpy's first maximum over the oracle's fp64 values.  The oracle row of a state is computed once, for
every column; a mask only overlays -inf."""
import numpy as np
import pytest
import torch

import best_order_cases as BC
import tap_net_amd as T
from tap_net_amd import _lib, generate, pack, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOFT, HARD = "C+P+S-lb-soft", "C+P+S-lb-hard"
# every instantiation: 2D widths 5, 12, 20, 40 and 3D 2x2, 4x4, 5x5, 8x8 -> G = 8, 16, 32, 64
SHAPES = [(2, [5, 50]), (2, [12, 50]), (2, [20, 50]), (2, [40, 50]),
          (3, [2, 2, 50]), (3, [4, 4, 50]), (3, [5, 5, 50]), (3, [8, 8, 50])]
# B = 1, 3, 67: no multiple of the containers a workgroup takes; n = 7: nR = 14 / 42, no multiple of the groups per wave
SIZES = [(67, 10), (3, 7), (1, 10)]


def _group(cs):
    cells = cs[0] * (cs[1] if len(cs) == 3 else 1)
    return 8 if cells <= 8 else 16 if cells <= 16 else 32 if cells <= 32 else 64


def _instances(B, n, D, cs, seed, sides=None):
    """synthetic precedence with block sides capped to what fits the container (a block that fits nowhere in an empty
    container scores 0 / 0); ``sides``: draw the sides from these values instead (ties on purpose)"""
    static, dynamic = synth.rand_instances(B, n, D, seed=seed)
    cap = float(min(cs[:-1] + [4]))
    static[:, 1:, :] = static[:, 1:, :].clamp(max=cap)
    if sides is not None:
        rng = np.random.RandomState(seed)
        base = rng.choice(sides, size=(B, n, D)).astype(np.float32)
        import itertools
        for r, p in enumerate(itertools.permutations(range(D))):
            for k in range(D):
                static[:, 1 + k, r * n:(r + 1) * n] = torch.from_numpy(base[:, :, p[k]])
    return static.contiguous(), dynamic


def _oracle_rows(cs, n, reward, committed, static):
    """(B, nR) float64: every column of every env tried on the oracle"""
    B, _, nR = static.shape
    out = np.empty((B, nR))
    for b in range(B):
        for c in range(nR):
            out[b, c] = BC.trial_score(cs, n, reward, committed[b], static[b, 1:, c].astype(np.int32))
    assert not np.isnan(out).any()
    return out


def _masked(full, mask):
    return np.where(mask != 0, full, -np.inf)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _trial_keys():
    return {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_TRIAL}


def _check_state(env, st, masks, full, stepped_too):
    """one state against its oracle row ``full`` under every mask of ``masks``; the blob must not change"""
    before = env._state.clone()
    tied = rows = 0
    for name, m in masks:
        scores, best = env.trial_scores(st, m)
        want = full if m is None else _masked(full, m.cpu().numpy())
        got = scores.cpu().numpy()
        assert _same_bits(got, want), name
        assert np.array_equal(best.cpu().numpy(), np.argmax(want, axis=1)), name
        if stepped_too:
            s2, b2 = env.trial_scores(st, m, stepped=True)
            assert _same_bits(s2.cpu().numpy(), got), name
            assert torch.equal(b2, best), name
        if name == "current":
            live = want.max(axis=1) > -np.inf
            rows += int(live.sum())
            tied += int(((want == want.max(axis=1, keepdims=True)).sum(axis=1) > 1)[live].sum())
    assert torch.equal(env._state, before), "trial_scores wrote to the state blob"
    return tied, rows


def _walk(D, cs, reward, B, n, seed, sides=None, stepped_too=True):
    """a random feasible episode, checked after 0, 1, 4 and n - 1 committed steps, then on the finished blob"""
    static, dynamic = _instances(B, n, D, cs, seed, sides)
    tape = synth.random_feasible_tape(static, dynamic, n, seed=seed + 1)
    st, dy = static.to(DEV), dynamic.to(DEV)
    st_np = static.numpy()
    env = T.BatchedContainer(B, cs, n, reward, "full", device=DEV)
    masks = pack.MaskStepper(st, dy)
    committed = [[] for _ in range(B)]
    tied = rows = 0
    fresh_rows = None
    _lib.variant_hits_reset(DEV)
    for t in range(n):
        if t in (0, 1, 4, n - 1):
            full = _oracle_rows(cs, n, reward, committed, st_np)
            if t == 0:
                fresh_rows = full
            cur = masks.current_mask
            zero_env = cur.clone()
            zero_env[B // 2] = 0                                  # one env with nothing selectable: best = 0
            single = cur.clone()
            single[0] = 0
            single[0, int(cur[0].argmax().item())] = 1            # one env holding a single column
            a, b = _check_state(env, st, [("none", None), ("current", cur), ("zero-env", zero_env), ("single", single)],
                                full, stepped_too)
            tied, rows = tied + a, rows + b
            s, best = env.trial_scores(st, zero_env)
            assert int(best[B // 2].item()) == 0 and bool(torch.isinf(s[B // 2]).all())
        ptr = tape[:, t].to(DEV)
        for b in range(B):
            committed[b].append(st_np[b, 1:, int(tape[b, t])].astype(np.int32))
        masks.step(ptr)
        env.add_new_blocks_gather(st, ptr, want_feature=False)
    env.check()
    # the finished blob: every further block is one too many (error bit 2) -> -1.0, and the error words stay clear
    before = env._state.clone()
    s, best = env.trial_scores(st)
    assert bool((s == -1.0).all()) and bool((best == 0).all())
    assert bool((env.errors == 0).all())
    # fresh=True on the stale blob = the scores of a reset container
    s, best = env.trial_scores(st, fresh=True)
    assert _same_bits(s.cpu().numpy(), fresh_rows)
    assert np.array_equal(best.cpu().numpy(), np.argmax(fresh_rows, axis=1))
    if stepped_too:
        s2, b2 = env.trial_scores(st, fresh=True, stepped=True)
        assert _same_bits(s2.cpu().numpy(), fresh_rows) and torch.equal(b2, best)
    assert torch.equal(env._state, before)
    hard = 1 if reward.endswith("hard") else 0
    keys = _trial_keys()
    G = _group(cs)
    for mask_given, fresh in ((0, 0), (1, 0), (0, 1)):
        assert (_lib.TAP_HIT_TRIAL, D, G, hard, mask_given, fresh, 0) in keys, keys
    return tied, rows


@pytest.mark.parametrize("reward", [SOFT, HARD])
@pytest.mark.parametrize("D,cs", SHAPES, ids=lambda v: "x".join(map(str, v[:-1])) if isinstance(v, list) else None)
def test_every_instantiation_against_oracle_and_stepped(D, cs, reward):
    for B, n in SIZES:
        _walk(D, cs, reward, B, n, seed=100 + 7 * B + n)


@pytest.mark.parametrize("D,cs", [(2, [5, 50]), (3, [4, 4, 50])])
def test_ties_take_the_first_maximum(D, cs):
    """square blocks (both rotations are the same block) and duplicated blocks: at least a quarter of the rows have a
    tied maximum, and the pick is numpy's first maximum over the oracle's fp64 values"""
    tied, rows = _walk(D, cs, SOFT, 24, 10, seed=5, sides=[1, 2], stepped_too=False)
    assert rows > 0 and tied * 4 >= rows, (tied, rows)


def test_refused_candidates_score_minus_one():
    """a container of height 6 and sides up to 5: late in the episode some candidates overflow -- they score -1.0, the
    envs' error words stay 0, and ``best`` avoids them while another column scores >= 0"""
    B, n, cs = 64, 6, [5, 6]
    rng = np.random.RandomState(11)
    static = np.zeros((B, 3, 2 * n), np.float32)
    sizes = rng.randint(1, 6, size=(B, n, 2)).astype(np.float32)
    static[:, 0] = np.tile(np.arange(n, dtype=np.float32), 2)
    static[:, 1, :n], static[:, 2, :n] = sizes[:, :, 0], sizes[:, :, 1]
    static[:, 1, n:], static[:, 2, n:] = sizes[:, :, 1], sizes[:, :, 0]
    st = torch.from_numpy(static).to(DEV)
    env = T.BatchedContainer(B, cs, n, SOFT, "full", device=DEV)
    left = torch.ones(B, 2 * n, device=DEV)
    committed = [[] for _ in range(B)]
    refused = avoided = 0
    for t in range(4):
        scores, best = env.trial_scores(st, left)
        want = _masked(_oracle_rows(cs, n, SOFT, committed, static), left.cpu().numpy())
        got = scores.cpu().numpy()
        assert _same_bits(got, want)
        assert np.array_equal(best.cpu().numpy(), np.argmax(want, axis=1))
        assert bool((env.errors == 0).all())
        s2, b2 = env.trial_scores(st, left, stepped=True)
        assert _same_bits(s2.cpu().numpy(), got) and torch.equal(b2, best)
        refused += int((got == -1.0).sum())
        pick = best.cpu().numpy()
        top = got[np.arange(B), pick]
        avoided += int(((got == -1.0).any(axis=1) & (top >= 0)).sum())
        assert not (top[(got >= 0).any(axis=1)] < 0).any()
        go = top >= 0                                             # an env whose every candidate overflows stops here
        for b in np.flatnonzero(go):
            committed[b].append(static[b, 1:, pick[b]].astype(np.int32))
        env.add_new_blocks_gather(st, best, active=torch.from_numpy(go).to(DEV), want_feature=False)
        blk = torch.from_numpy(np.where(go, pick % n, -1)).to(DEV)
        for r in range(2):
            cols = (blk + r * n).clamp(min=0)
            left[torch.arange(B, device=DEV)[blk >= 0], cols[blk >= 0]] = 0
    assert refused > 0 and avoided > 0
    assert bool((env.errors == 0).all())
    env.check()


def test_arguments_and_fallback():
    B, n = 5, 6
    static, dynamic = _instances(B, n, 2, [5, 50], 3)
    st = static.to(DEV)
    with pytest.raises(T.TapError) as ei:
        T.BatchedContainer(B, [5, 50], n, "C+P+S-SL-soft", "full", device=DEV, place_at='container').trial_scores(st)
    assert ei.value.status == _lib.TAP_E_INVALID
    env = T.BatchedContainer(B, [5, 50], n, SOFT, "full", device=DEV)
    with pytest.raises(ValueError):
        env.trial_scores(st, out=torch.empty(B, 2 * n, device=DEV))                      # float32: not the fp64 scores
    with pytest.raises(ValueError):
        env.trial_scores(st, mask=torch.ones(B, n, device=DEV))
    out = torch.empty(B, 2 * n, dtype=torch.float64, device=DEV)
    best = torch.empty(B, dtype=torch.int64, device=DEV)
    s, b = env.trial_scores(st, out=out, best_out=best)
    assert s is out and b is best
    # strategies and sizes beyond the one-launch kernel answer through the stepped form
    for cs, reward, D in (([5, 50], "C+P+S-mcs-soft", 2), ([70, 50], SOFT, 2), ([9, 4, 50], SOFT, 3)):
        static, dynamic = _instances(B, n, D, cs, 4)
        st = static.to(DEV)
        e = T.BatchedContainer(B, cs, n, reward, "full", device=DEV)
        _lib.variant_hits_reset(DEV)
        s, b = e.trial_scores(st)
        assert not _trial_keys()
        want = _oracle_rows(cs, n, reward, [[] for _ in range(B)], static.numpy())
        assert _same_bits(s.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), np.argmax(want, axis=1))
    with pytest.raises(NotImplementedError):
        T.BestRatioPolicy(env)(step=0, static=torch.zeros(B, 4, 2 * n, device=DEV), current_mask=torch.ones(B, 2 * n, device=DEV))


def _groups():
    groups = {}
    for c in BC.CASES:
        groups.setdefault((tuple(c.initial), tuple(c.target), c.n, c.reward_type, c.allow_bot), []).append(c)
    return list(groups.items())


@pytest.mark.parametrize("key,cases", _groups(), ids=lambda v: v[0].id if isinstance(v, list) else None)
def test_best_orders_reproduce_the_reference(key, cases):
    """generate.best_orders on every fixture case, batched by shape: the reference's solution exactly,
    mean_valid_nodes_num to 1e-12; the mcs / mul cases run through the stepped form"""
    init, target, n, reward, allow_bot = key
    blocks = torch.from_numpy(np.stack([c.blocks for c in cases])).to(DEV)
    positions = torch.from_numpy(np.stack([c.positions for c in cases])).to(DEV)
    _lib.variant_hits_reset(DEV)
    tours, mean_valid = generate.best_orders(blocks, positions, list(init), list(target), reward, 1, allow_bot)
    assert tours.dtype == torch.int64 and mean_valid.dtype == torch.float64
    assert tours.cpu().numpy().tolist() == [c.solution for c in cases]
    assert np.abs(mean_valid.cpu().numpy() - np.asarray([c.mean_valid for c in cases])).max() <= 1e-12
    assert bool(_trial_keys()) == cases[0].lane_kernel


@pytest.mark.parametrize("case", BC.CASES, ids=lambda c: c.id)
def test_generate_order_graph_facade(case):
    solution, search_time, mean_valid = generate.generate_order_graph(
        case.blocks, case.positions, case.initial, 1, case.allow_bot, 'best', case.reward_type, case.target)
    assert solution == case.solution and all(isinstance(v, int) for v in solution)
    assert abs(mean_valid - case.mean_valid) <= 1e-12 and search_time > 0


@pytest.mark.parametrize("fused", [True, False])
def test_policy_on_both_loops(fused):
    """run_episode(..., env=env, policy=BestRatioPolicy(env)) on the fused stepper and on the two-launch loop: the
    tour of the oracle's greedy loop"""
    cases = [c for c in BC.CASES if c.initial == [5, 50] and c.n == 10 and c.reward_type == SOFT and c.allow_bot]
    blocks = torch.from_numpy(np.stack([c.blocks for c in cases])).to(DEV)
    positions = torch.from_numpy(np.stack([c.positions for c in cases])).to(DEV)
    st, dy = generate.precedence_tensors(blocks, positions, [5, 50])
    env = T.BatchedContainer(len(cases), [5, 50], 10, SOFT, "diff", device=DEV)
    out = T.run_episode(st, dy, T.BestRatioPolicy(env), 5, 50, reward_type=SOFT, env=env, fused=fused)
    assert out["tour_idx"].cpu().numpy().tolist() == [c.solution for c in cases]
    env.check()


def test_episode_replays_from_a_hip_graph():
    """one episode under BestRatioPolicy captured at 2D W = 5, n = 10, B = 64 and replayed on two fresh instance sets:
    the trial call allocates nothing, reads nothing back and does not synchronise"""
    B, n = 64, 10
    sets = [_instances(B, n, 2, [5, 50], seed) for seed in (21, 22, 23)]
    st, dy = sets[0][0].to(DEV), sets[0][1].to(DEV)
    env = T.BatchedContainer(B, [5, 50], n, SOFT, "diff", device=DEV)
    pol = T.BestRatioPolicy(env)
    pack.set_binary_check('trust')
    try:
        run = lambda: T.run_episode(st, dy.clone(), pol, 5, 50, reward_type=SOFT, env=env)      # noqa: E731
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = run()
        tours = []
        for static, dynamic in sets[1:]:
            st.copy_(static)
            dy.copy_(dynamic)
            graph.replay()
            torch.cuda.synchronize()
            got_tour, got_reward = rec["tour_idx"].clone(), rec["reward"].clone()
            eager = run()
            assert torch.equal(got_tour, eager["tour_idx"]) and torch.equal(got_reward, eager["reward"])
            tours.append(got_tour.cpu().numpy())
        assert not np.array_equal(tours[0], tours[1])
        env.check()
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
