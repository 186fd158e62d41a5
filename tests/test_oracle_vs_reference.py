"""Differential test: CPU oracle vs the reference's full state after every step, including the voxel grid.

The reference's side is recorded in tests/golden/reference_diff.npz (tests/golden/make_golden.py --only
reference_diff runs the reference over exactly the cases listed here); the blocks are regenerated from the seeds.
"""
import numpy as np
import pytest

import golden_util as G
import oracle_lib as O

# test name -> (reward types, runs of (cs, n, feat, strategy, episodes, seed, lo, hi, hz))
DIFF_CASES = {
    "lbg2d": (["C+P+S-lb-soft", "C+P+S-lb-hard", "C+P-lb-soft", "C+P-lb-hard"], [
        ([5, 50], 10, "diff", "LB_GREEDY", 60, 11, 1, 5, None),
        ([7, 100], 20, "zero", "LB_GREEDY", 20, 12, 1, 5, None),
        ([3, 60], 8, "full", "LB_GREEDY", 20, 13, 1, 6, None)]),
    "lbg3d": (["C+P+S-lb-soft", "C+P+S-lb-hard"], [
        ([5, 5, 50], 10, "diff", "LB_GREEDY", 40, 21, 1, 5, None),
        ([5, 5, 250], 30, "full", "LB_GREEDY", 6, 22, 1, 5, None),
        ([6, 6, 80], 12, "diff", "LB_GREEDY", 12, 23, 1, 7, None)]),
    # packing_strategy 'LB' (tools.py:3683-3686, :1602-1955)
    "lb_legacy": (["C+P+S-lb-soft", "C+P+S-lb-hard", "C+P-lb-soft"], [
        ([5, 50], 10, "diff", "LB", 40, 51, 1, 5, None),
        ([7, 100], 20, "zero", "LB", 10, 52, 1, 5, None),
        ([3, 60], 8, "full", "LB", 15, 53, 1, 6, None),
        ([5, 5, 50], 10, "diff", "LB", 20, 54, 1, 5, None),
        ([4, 6, 80], 12, "full", "LB", 6, 55, 1, 6, None)]),
    "macs2d": (["C+P+S-mcs-soft", "C+P+S-mcs-hard", "C+P+S-mul-soft", "C+P-mcs-soft"], [
        ([7, 100], 20, "diff", "MACS", 25, 31, 1, 5, None),
        ([5, 50], 10, "diff", "MACS", 40, 32, 1, 5, None),
        # wide containers (the kernels' 32- and 64-lane form, tap_macs_wide.h), blocks up to 8 wide
        ([20, 60], 24, "diff", "MACS", 4, 33, 1, 7, None),
        ([40, 40], 30, "full", "MACS", 2, 34, 1, 9, None),
        ([64, 30], 24, "zero", "MACS", 2, 35, 1, 9, None),
        # above 64 columns (the kernels' one-thread-per-container form, macs_big.hip), blocks up to 70 wide
        ([100, 40], 30, "diff", "MACS", 2, 36, 1, 14, None),
        ([70, 60], 16, "full", "MACS", 2, 37, 1, 30, 7),
        ([130, 50], 12, "zero", "MACS", 1, 38, 2, 71, 6)]),
    "macs3d": (["C+P+S-mcs-soft", "C+P+S-mcs-hard", "C+P+S-mul-soft", "mcs-soft"], [
        ([5, 5, 50], 10, "diff", "MACS", 12, 41, 1, 5, None),
        ([6, 6, 60], 16, "full", "MACS", 4, 42, 1, 6, None),
        ([4, 7, 40], 12, "diff", "MACS", 4, 43, 1, 5, None),
        # above 64 cells / sides above 8 (the kernels' one-thread-per-container form, macs3_big.hip), footprints up to 8 x 8
        ([10, 10, 40], 24, "diff", "MACS", 2, 44, 1, 6, None),
        ([12, 9, 30], 20, "full", "MACS", 1, 45, 1, 9, 5),
        ([9, 16, 30], 20, "zero", "MACS", 1, 46, 2, 8, 6)]),
}

MASK_SHAPES = [(32, 6, 2), (16, 30, 2), (8, 42, 6), (8, 22, 6)]   # (B, n, R): 18 .. 126 rows


def diff_key(cs, n, reward, feat, strategy, episodes, seed, lo, hi, hz):
    return repr((list(cs), n, reward, feat, strategy, episodes, seed, lo, hi, hz))


def diff_blocks(cs, n, episodes, seed, lo, hi, hz):
    """The blocks of every episode of one run, (episodes, n, D)."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(episodes):
        blocks = rng.randint(lo, hi, size=(n, len(cs)))
        if hz is not None:                                   # wide blocks, heights below hz
            blocks[:, -1] = rng.randint(1, hz, size=n)
        out.append(blocks)
    return np.asarray(out)


def mask_inputs(shape):
    B, n, R = shape
    rng = np.random.RandomState(5)
    dyn = (rng.rand(B, 3 * n, n * R) < 0.12).astype(np.float32)
    static = np.zeros((B, 3 if R == 2 else 4, n * R), np.float32)     # 1 + D rows: pack.py reads D off the shape
    static[:, 0, :] = np.tile(np.arange(n), R)
    mask = (rng.rand(B, n * R) < 0.8).astype(np.float32)
    ptr = rng.randint(0, n * R, size=B).astype(np.int64)
    return dyn, static, mask, ptr


def reward_mul_inputs(D):
    rng = np.random.RandomState(17 + D)
    B, n = 24, 8
    R = 2 if D == 2 else 6
    blocks = rng.randint(1, 5, size=(B, D, n)).astype(np.float32)
    static = np.zeros((B, 1 + D + 1, n * R), np.float32)
    for r in range(R):
        static[:, 0, r * n:(r + 1) * n] = np.arange(n)
        static[:, 1:1 + D, r * n:(r + 1) * n] = blocks          # same sides in every rotation slot: enough here
        static[:, -1, r * n:(r + 1) * n] = rng.randint(0, 2, size=(B, n))
    static[0, -1, :] = 0                                         # one env with an empty second container
    tour = np.stack([rng.permutation(n * R)[:n] for _ in range(B)]).astype(np.int64)
    return static, tour, R


@pytest.fixture(scope="module")
def rec():
    return G.load("reference_diff.npz")


def _diff(rec, reward, cs, n, feat, strategy, episodes, seed, lo, hi, hz):
    k = G.key_index(rec, diff_key(cs, n, reward, feat, strategy, episodes, seed, lo, hi, hz))
    want = {f: rec["k%d_%s" % (k, f)] for f in ("features", "heightmap", "positions", "stable", "valid", "empty",
                                                 "container", "ratio")}
    for ep, blocks in enumerate(diff_blocks(cs, n, episodes, seed, lo, hi, hz)):
        o = O.Env(cs, n, reward, feat, strategy)
        for t in range(n):
            rc, of = o.add_new_block(blocks[t])
            ctx = (cs, reward, strategy, ep, t, blocks[: t + 1].tolist())
            assert rc == 0, ctx
            assert np.array_equal(want["features"][ep, t], of), ctx
            assert np.array_equal(want["heightmap"][ep, t], o.heightmap), ctx
            assert np.array_equal(want["positions"][ep, t], o.positions), ctx
            assert want["stable"][ep, t].tolist() == o.stable.tolist(), ctx
            assert want["valid"][ep, t] == o.valid_size and want["empty"][ep, t] == o.empty_size, ctx
            assert np.array_equal(want["container"][ep, t], o.container), ctx
        a, b = float(want["ratio"][ep]), o.calc_ratio()
        assert a == b or (np.isnan(a) and np.isnan(b))


def _run(rec, name, reward):
    for run in DIFF_CASES[name][1]:
        _diff(rec, reward, *run)


@pytest.mark.parametrize("reward", DIFF_CASES["lbg2d"][0])
def test_lbg2d(rec, reward):
    _run(rec, "lbg2d", reward)


@pytest.mark.parametrize("reward", DIFF_CASES["lbg3d"][0])
def test_lbg3d(rec, reward):
    _run(rec, "lbg3d", reward)


@pytest.mark.parametrize("reward", DIFF_CASES["lb_legacy"][0])
def test_lb_legacy(rec, reward):
    """packing_strategy 'LB' (tools.py:3683-3686, :1602-1955), full state incl. the voxel grid."""
    _run(rec, "lb_legacy", reward)


@pytest.mark.parametrize("reward", DIFF_CASES["macs2d"][0])
def test_macs2d(rec, reward):
    _run(rec, "macs2d", reward)


@pytest.mark.parametrize("reward", DIFF_CASES["macs3d"][0])
def test_macs3d(rec, reward):
    _run(rec, "macs3d", reward)


@pytest.mark.parametrize("shape", MASK_SHAPES)
def test_masks(rec, shape):
    """pack.update_dynamic / pack.update_mask on random (not necessarily feasible) tensors."""
    dyn, static, mask, ptr = mask_inputs(shape)
    B, n, R = shape
    od = O.update_dynamic(dyn, static, ptr, n, 3)
    oc, om = O.update_mask(mask, od, ptr, n, R)
    pre = "masks_%d_%d_%d_" % shape
    assert np.array_equal(rec[pre + "dynamic"], od)
    assert np.array_equal(rec[pre + "current_mask"], oc) and np.array_equal(rec[pre + "mask"], om)


@pytest.mark.parametrize("D", [2, 3])
def test_reward_mul(rec, D):
    """pack.reward for the two-container input type: blocks split by target id, packed separately."""
    static, tour, R = reward_mul_inputs(D)
    got = O.reward_mul(static, tour, "C+P+S-lb-soft", 5, 60, R)
    want = rec["reward_mul_%dd" % D]
    assert np.array_equal(got, want)
