"""LB_GREEDY on containers of 4 097 .. 16 384 cells (one workgroup per container, big.hip: k_big_wg_step /
k_big_wg_episode): per step and whole episodes against the CPU oracle, and -- for 2D widths above the oracle's 4 096
columns -- against the reference's own traces (tests/golden/big_lbg.npz, make_golden_big.py).  Every shape here was
refused with TAP_E_UNSUPPORTED before."""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_lbg.npz")


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


def _feat_np(f):
    return f.detach().cpu().numpy().reshape(f.shape[0], -1).astype(np.int64)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _blocks(rs, B, n, D, lo, hi, hmax=6):
    b = rs.randint(lo, hi, size=(B, n, D)).astype(np.int32)
    b[:, :, -1] = rs.randint(1, hmax, size=(B, n))
    return b


# (container, block sides [lo, hi), B, n); the last two: 3D sides of 9 .. 16 (the wide stability path)
STEP_SHAPES = [([65, 65, 40], (1, 13), 33, 7), ([100, 100, 60], (2, 17), 17, 6), ([128, 128, 40], (3, 17), 19, 6),
               ([100, 41, 50], (1, 12), 65, 7), ([128, 128, 30], (9, 17), 17, 6), ([70, 70, 40], (9, 17), 130, 6)]


@pytest.mark.parametrize("reward", ["C+P+S-lb-soft", "C+P+S-lb-hard"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=lambda s: "x".join(map(str, s[0])))
def test_steps_vs_oracle(T, shape, reward):
    """BatchedContainer.add_new_blocks step by step: positions, height-maps, stable flags, counters, all three
    features bit-exact; calc_ratio bit-exact"""
    cs, (lo, hi), B, n = shape
    D = len(cs)
    rs = np.random.RandomState(cs[0] * 7 + cs[1] + n)
    blocks = _blocks(rs, B, n, D, lo, hi)
    blocks[0, :, :2] = 16                                                         # footprints at the wide limit
    blk = torch.as_tensor(blocks, device=DEV)
    for feat in ("diff", "zero", "full"):
        ref = O.run_episodes(O.make_desc(cs, n, reward, feat), blocks, nthreads=8)
        assert ref["nerr"] == 0
        env = T.BatchedContainer(B, cs, n, reward, feat, device=DEV)
        assert not env.fused_ok
        for t in range(n):
            f = _feat_np(env.add_new_blocks(blk[:, t].contiguous()))
            assert np.array_equal(f, ref["features"][:, t]), (feat, t)
            assert np.array_equal(env.heightmap.cpu().numpy().reshape(B, -1), ref["heightmaps"][:, t]), (feat, t)
        env.check()
        assert np.array_equal(env.positions.cpu().numpy(), ref["positions"])
        assert np.array_equal(env.stable.cpu().numpy().astype(np.uint8), ref["stable"])
        assert np.array_equal(env.valid_size.cpu().numpy(), ref["counters"][:, 0])
        assert np.array_equal(env.empty_size.cpu().numpy(), ref["counters"][:, 1])
        assert np.array_equal(_bits(env.calc_ratios64().cpu().numpy()), _bits(ref["ratio"]))
        assert np.allclose(env.calc_ratios().cpu().numpy(), ref["ratio"], rtol=0, atol=1e-6)
        assert np.array_equal(_feat_np(env.get_heightmaps()), ref["features"][:, n - 1])


def test_overflow_and_bad_blocks_flagged(T):
    """error bits at these sizes: a block above H, a 3D side above 16 (bit 4) and too many steps"""
    cs, n, B = [100, 100, 12], 3, 5
    blocks = np.ones((B, n + 1, 3), np.int32) * 4
    blocks[1, 1] = [5, 5, 20]                                                     # z + bz > H
    blocks[2, 0] = [17, 3, 2]                                                     # side beyond the wide support test
    env = T.BatchedContainer(B, cs, n, "C+P+S-lb-hard", "diff", device=DEV)
    blk = torch.as_tensor(blocks, device=DEV)
    for t in range(n + 1):
        env.add_new_blocks(blk[:, t].contiguous())
    err = env.errors.cpu().numpy()
    assert err[1] & 1 and err[2] & 4 and (err[[0, 1, 3, 4]] & 2).all()         # (container 2 took one step less)
    with pytest.raises(T.TapError):
        env.check()


def test_2d_wide_containers_vs_reference(T):
    """2D containers of 5 000 and 16 384 columns (beyond the oracle's 4 096): the reference's traces, stepped and
    whole-episode, plus per-step height-maps / features rebuilt from its positions"""
    from tap_net_amd import generate as gen
    z = np.load(GOLDEN)
    for case in [c for c in z["cases"] if str(c).startswith("w")]:
        cs = [int(v) for v in z[case + "_cs"]]
        reward = str(z[case + "_reward"])
        blocks, want_pos, want_st = z[case + "_blocks"], z[case + "_positions"], z[case + "_stable"]
        E, n, _ = blocks.shape
        W = cs[0]
        blk = torch.as_tensor(blocks, device=DEV)
        for feat in ("diff", "zero", "full"):
            env = T.BatchedContainer(E, cs, n, reward, feat, device=DEV)
            hm = np.zeros((E, W), np.int64)
            for t in range(n):
                f = _feat_np(env.add_new_blocks(blk[:, t].contiguous()))
                for e in range(E):
                    x, zz = want_pos[e, t]
                    if t == 0 or want_pos[e, t].any() or want_st[e, t]:
                        hm[e, x:x + blocks[e, t, 0]] = zz + blocks[e, t, 1]
                assert np.array_equal(env.heightmap.cpu().numpy().reshape(E, -1), hm), (case, t)
                want_f = np.diff(hm, axis=1) if feat == "diff" else hm - (hm.min(1, keepdims=True) if feat == "zero" else 0)
                assert np.array_equal(f, want_f), (case, feat, t)
            env.check()
            assert np.array_equal(env.positions.cpu().numpy(), want_pos), case
            assert np.array_equal(env.stable.cpu().numpy().astype(np.uint8), want_st), case
            cps = env.calc_CPS().cpu().numpy()                                    # calc_positions_lb_greedy's C + P + S
            assert np.allclose((cps[:, 0] + cps[:, 1]) + cps[:, 2], z[case + "_ratio"], rtol=0, atol=1e-12)
        pos, st, rew = gen.pack_blocks(blk, cs, reward)
        assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(st.cpu().numpy().astype(np.uint8), want_st)
        assert np.allclose(-rew.cpu().numpy().astype(np.float64), z[case + "_ratio"], rtol=0, atol=1e-6)
        pos_s, st_s, rew_s = gen._pack_blocks_stepped(blk, cs, reward, torch.device(DEV))
        assert torch.equal(pos_s, pos) and torch.equal(st_s, st) and torch.equal(rew_s, rew)


def test_3d_golden_vs_library(T):
    """the reference's 70 x 70 traces through generate.pack_blocks"""
    from tap_net_amd import generate as gen
    z = np.load(GOLDEN)
    for case in [c for c in z["cases"] if str(c).startswith("c")]:
        cs = [int(v) for v in z[case + "_cs"]]
        pos, st, rew = gen.pack_blocks(torch.as_tensor(z[case + "_blocks"], device=DEV), cs, str(z[case + "_reward"]))
        assert np.array_equal(pos.cpu().numpy(), z[case + "_positions"]), case
        assert np.array_equal(st.cpu().numpy().astype(np.uint8), z[case + "_stable"]), case
        assert np.allclose(-rew.cpu().numpy().astype(np.float64), z[case + "_ratio"], rtol=0, atol=1e-6)


EPISODE_CFGS = [([100, 100, 60], (2, 17), "C+P+S-lb-soft", 37, 8), ([128, 128, 40], (3, 17), "C+P+S-lb-hard", 21, 8),
                ([65, 65, 40], (9, 17), "C+P+S-lb-hard", 66, 6), ([100, 41, 50], (1, 12), "C+P-lb-soft", 40, 9),
                ([5000, 60], (100, 900), "C+P+S-lb-soft", 24, 8), ([16384, 40], (300, 3000), "C+P+S-lb-hard", 16, 8)]


@pytest.mark.parametrize("cfg", EPISODE_CFGS, ids=lambda c: "x".join(map(str, c[0])) + "-" + c[2])
def test_whole_episodes(T, cfg):
    """tap_pack_blocks / tap_episode_reward / tap_episode_scores in one launch: against the oracle (3D) and against
    the stepped path of the same library (all shapes)"""
    from tap_net_amd import generate as gen, pack
    cs, (lo, hi), reward, B, n = cfg
    D = len(cs)
    rs = np.random.RandomState(B + n + cs[0])
    blocks = _blocks(rs, B, n, D, lo, hi, 5)
    bt = torch.as_tensor(blocks, device=DEV)
    pos, stable, rew = gen.pack_blocks(bt, cs, reward)
    pos_s, stable_s, rew_s = gen._pack_blocks_stepped(bt, cs, reward, torch.device(DEV))
    assert torch.equal(pos_s, pos) and torch.equal(stable_s, stable) and torch.equal(rew_s, rew)
    if D == 3:
        want = O.run_episodes(O.make_desc(cs, n, reward, "full"), blocks, nthreads=8, want_features=False, want_heightmaps=False)
        assert want["nerr"] == 0
        assert np.array_equal(pos.cpu().numpy(), want["positions"])
        assert np.array_equal(stable.cpu().numpy().astype(np.uint8), want["stable"])
        cps = want["cps"]
        assert np.array_equal(rew.cpu().numpy(), -((cps[:, 0] + cps[:, 1]) + cps[:, 2]).astype(np.float32))
    # the tour forms: static in PACKDataset's layout, one permutation per container
    import itertools
    R = 2 if D == 2 else 6
    static = torch.zeros(B, 1 + D, n * R, device=DEV)
    static[:, 0] = torch.arange(n, device=DEV).repeat(R)
    bf = torch.as_tensor(blocks, device=DEV, dtype=torch.float32)
    for r, perm in enumerate(itertools.permutations(range(D))):
        for k in range(D):
            static[:, 1 + k, r * n:(r + 1) * n] = bf[:, :, perm[k]]
    tour = torch.stack([torch.randperm(n * R, generator=torch.Generator().manual_seed(b))[:n] for b in range(B)]).to(DEV)
    stn, tn = static.cpu().numpy(), tour.cpu().numpy()
    bl2 = np.stack([stn[np.arange(B), 1:, tn[:, t]] for t in range(n)], axis=1).astype(np.int32)
    p2, s2, r2 = gen._pack_blocks_stepped(torch.as_tensor(bl2, device=DEV), cs, reward, torch.device(DEV))
    ok = ~torch.isnan(r2).cpu().numpy()
    ratio, scores = pack.episode_scores(static, tour, reward, "bot", True, cs, check=False)
    assert np.allclose(ratio.cpu().numpy()[ok], -r2.cpu().numpy().astype(np.float64)[ok], rtol=0, atol=1e-6)
    if D == 2 or cs[0] == cs[1]:
        got = pack.reward(static, tour, reward, "bot", True, cs[0], cs[-1])
        assert np.array_equal(got.cpu().numpy()[ok], r2.cpu().numpy()[ok])
    if D == 3:
        want2 = O.run_episodes(O.make_desc(cs, n, reward, "full"), bl2, nthreads=8, want_features=False, want_heightmaps=False)
        good = want2["errs"] == 0
        c2 = want2["cps"]
        assert np.array_equal(_bits(ratio.cpu().numpy()[good]), _bits(((c2[:, 0] + c2[:, 1]) + c2[:, 2])[good]))
        assert np.array_equal(scores.cpu().numpy()[good, 0], want2["counters"][good, 0])


def test_size_boundaries(T):
    """4 096 cells take the one-wavefront kernels as before, 16 384 are accepted, 16 385 raise TAP_E_UNSUPPORTED"""
    from tap_net_amd import _lib, generate as gen
    rs = np.random.RandomState(4)
    for cs, lo, hi in (([64, 64, 40], 1, 12), ([4096, 40], 50, 600), ([128, 128, 40], 2, 16), ([16384, 40], 50, 2000)):
        D = len(cs)
        blocks = _blocks(rs, 9, 5, D, lo, hi)
        pos, st, rew = gen.pack_blocks(torch.as_tensor(blocks, device=DEV), cs, "C+P+S-lb-hard")
        if cs[0] <= 4096 or D == 3:
            want = O.run_episodes(O.make_desc(cs, 5, "C+P+S-lb-hard", "full"), blocks, want_features=False, want_heightmaps=False)
            assert want["nerr"] == 0
            assert np.array_equal(pos.cpu().numpy(), want["positions"]), cs
    for cs in ([16385, 40], [128, 129, 40], [200, 100, 40]):
        with pytest.raises(T.TapError) as ei:
            T.BatchedContainer(4, cs, 5, "C+P+S-lb-soft", "diff", device=DEV).add_new_blocks(
                torch.ones(4, len(cs), dtype=torch.int32, device=DEV))
        assert ei.value.status == _lib.TAP_E_UNSUPPORTED
        assert "16384" in str(ei.value)


def test_create_dataset_and_unit_scaled_dataset(T, tmp_path, monkeypatch):
    """create_dataset with a 70 x 70 initial container (hard LB_GREEDY inside the generator's acceptance loop), then
    PACKDataset(unit=10) of a width-7 set: a 70 x 70 container for pack.reward"""
    from tap_net_amd import generate as gen, pack
    monkeypatch.chdir(tmp_path)
    st, dy, bl, ps = gen.generate_instances(64, 8, 3, 70, 40, 1, (1, 9), seed=3, device=DEV, return_aux=True)
    pos2, stable2, _ = gen.pack_blocks(bl, [70, 70, 40])
    assert bool(stable2.all()) and torch.equal(pos2, ps)
    want = O.run_episodes(O.make_desc([70, 70, 40], 8, "C+P+S-lb-hard", "full"), bl.cpu().numpy(), want_features=False,
                          want_heightmaps=False)
    assert np.array_equal(ps.cpu().numpy(), want["positions"])
    # sizes 1 only: scaled by unit = 10 they stay within the 16-cell 3D sides the library supports
    train_dir, _ = pack.create_dataset(8, 32, 8, 3, 7, 50, 1, (1, 2), seed=11, device=DEV)
    ds = pack.PACKDataset(os.path.join(train_dir, ""), 8, 32, 1, "bot", "full", True, 7, unit=10)
    static = torch.stack([ds[i][0] for i in range(len(ds))]).to(DEV)
    B, n = static.shape[0], 8
    tour = torch.stack([torch.randperm(n * 6, generator=torch.Generator().manual_seed(b))[:n] for b in range(B)]).to(DEV)
    got = pack.reward(static, tour, "C+P+S-lb-soft", "bot", True, 70, 500)
    stn, tn = static.cpu().numpy(), tour.cpu().numpy()
    bl2 = np.stack([stn[np.arange(B), 1:, tn[:, t]] for t in range(n)], axis=1).astype(np.int32)
    assert bl2.min() == 10                                                        # sides scaled by unit
    w = O.run_episodes(O.make_desc([70, 70, 500], n, "C+P+S-lb-soft", "full"), bl2, want_features=False, want_heightmaps=False)
    assert w["nerr"] == 0
    c = w["cps"]
    assert np.array_equal(got.cpu().numpy(), -((c[:, 0] + c[:, 1]) + c[:, 2]).astype(np.float32))
