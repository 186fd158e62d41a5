"""The step seam (tap-net_amd/csrc/tap_step_seam.h) of the kernels in which one thread, wavefront or workgroup owns a
container: block fetch (i32 array, f32 array, gather from `static`), the `active` mask, admission (error bit 2 for a
full container, bit 4 for a bad block, each family's own limit), the commit and the feature -- on the smallest shapes
that reach each kernel, step by step against the CPU oracle.  A container that is idle or refused must keep its state
and still report its feature; the expected error bits are written out here from the three family rules, not read back
from the library.  The thread-per-container fallbacks take the same cases in one child process
(TAP_NO_WAVE_KERNELS=1)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_lib as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_MAX, STEPS = 4, 5                                  # the fifth step meets a full container: bit 2
WIDE_MAX_SIDE = 16                                   # tap_stable_wide.h


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


def _family_rejects(strategy, cs, blk):
    """the three family rules beyond "every side >= 1" """
    if len(cs) == 2:
        return False                                                              # MACS 2D, LB_GREEDY 2D, legacy LB 2D: nothing
    bx, by = int(blk[0]), int(blk[1])
    W, L = cs[0], cs[1]
    if strategy == "LB_GREEDY":                                                   # a side above 16 THAT FITS
        return (bx > WIDE_MAX_SIDE or by > WIDE_MAX_SIDE) and bx <= W and by <= L
    if strategy == "MACS":
        return bx > W or by > L or bx > WIDE_MAX_SIDE or by > WIDE_MAX_SIDE
    return False                                                                  # legacy LB


# (kernel the shape reaches, container, reward, strategy, B, largest footprint side + 1)
CASES = [("k_big_wave_step-soft", [65, 30], "C+P+S-lb-soft", "LB_GREEDY", 5, 9),
         ("k_big_wave_step-hard", [9, 8, 20], "C+P+S-lb-hard", "LB_GREEDY", 5, 5),
         ("k_big_wave_step-17", [20, 18, 20], "C+P+S-lb-soft", "LB_GREEDY", 5, 5),
         ("k_big_wg_step-2d", [4100, 30], "C+P+S-lb-hard", "LB_GREEDY", 3, 300),
         ("k_big_wg_step-3d", [65, 65, 20], "C+P+S-lb-soft", "LB_GREEDY", 3, 9),
         ("k_macs2d_wave_step", [66, 30], "mcs-soft", "MACS", 5, 9),
         ("k_macs3d_wave_step", [9, 9, 20], "C+P+S-mcs-soft", "MACS", 5, 5),
         ("k_lb_step-2d", [5, 20], "C+P+S-lb-soft", "LB", 5, 4),
         ("k_lb_step-3d", [4, 4, 16], "C+P+S-lb-hard", "LB", 5, 3)]
SOURCES = ["i32", "f32", "gather"]


def _plan(case):
    """blocks (B, STEPS, D), the active masks (STEPS, B) and, per family, its bad blocks"""
    name, cs, reward, strategy, B, hi = case
    D = len(cs)
    rs = np.random.RandomState(len(name) * 131 + cs[0])
    blocks = rs.randint(1, hi, size=(B, STEPS, D)).astype(np.int32)
    blocks[:, :, -1] = rs.randint(1, 4, size=(B, STEPS))                          # heights 1 .. 3: nothing reaches H
    active = np.ones((STEPS, B), bool)
    for t in range(STEPS):
        active[t, (t + np.arange(B)) % 3 == 0] = False                            # about a third idle on every step
    active[:, 0] = True                                                           # container 0 takes all five: bit 2 on the last
    blocks[1, 1, 0] = 0                                                           # a zero side, every family
    if D == 3 and strategy == "LB_GREEDY" and cs[0] > WIDE_MAX_SIDE:
        blocks[2, 0, :2] = [17, 2]                                                # a side of 17 that fits
    if D == 3 and strategy == "MACS":
        blocks[2, 0, :2] = [cs[0] + 1, 2]                                         # bx > W
    active[0, 2] = active[1, 1] = True                                            # the bad blocks are looked at
    return blocks, active


def _feat_np(f):
    return f.detach().cpu().numpy().reshape(f.shape[0], -1).astype(np.int64)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _state(env):
    cnt = env.counters.cpu().numpy()
    return dict(hm=env.heightmap.cpu().numpy().reshape(env.batch_size, -1), pos=env.positions.cpu().numpy(),
                stable=env.stable.cpu().numpy().astype(np.uint8), cnt=cnt, ratio=env.calc_ratios64().cpu().numpy())


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_step_seam_vs_oracle(T, case, source):
    name, cs, reward, strategy, B, hi = case
    D = len(cs)
    blocks, active = _plan(case)
    nR = 7
    rs = np.random.RandomState(5)
    # gather: column ptr[b] of static holds the step's block; one ptr outside [0, nR) -- all sides 0 to the kernel
    static = rs.randint(1, 4, size=(STEPS, B, 1 + D, nR)).astype(np.float32)
    ptr = rs.randint(0, nR, size=(STEPS, B)).astype(np.int64)
    for t in range(STEPS):
        static[t, np.arange(B), 1:, ptr[t]] = blocks[:, t]
    bad_ptr = (3, B - 1)                                                          # (step, container)
    ptr[bad_ptr] = nR + 2 if source == "gather" else ptr[bad_ptr]
    active[3, B - 1] = True
    seen_blocks = np.stack([static[t, np.arange(B), 1:, np.clip(ptr[t], 0, nR - 1)] for t in range(STEPS)], axis=1).astype(np.int32)
    assert np.array_equal(seen_blocks[ptr.T < nR], blocks[ptr.T < nR])            # the host-side gather feeds the oracle
    if source == "gather":
        seen_blocks[bad_ptr[1], bad_ptr[0]] = 0
    else:
        seen_blocks = blocks
    for feat in ("diff", "zero", "full"):
        orc = [O.Env(cs, N_MAX, reward, feat, strategy) for _ in range(B)]
        env = T.BatchedContainer(B, cs, N_MAX, reward, feat, packing_strategy=strategy, device=DEV)
        assert not env.fused_ok
        want_err = np.zeros(B, np.int32)
        count = np.zeros(B, np.int64)
        nstable = np.zeros(B, np.int64)
        for t in range(STEPS):
            before = _state(env)
            act = torch.as_tensor(active[t], device=DEV)
            if source == "gather":
                f = env.add_new_blocks_gather(torch.as_tensor(static[t], device=DEV), torch.as_tensor(ptr[t], device=DEV), active=act)
            else:
                b = torch.as_tensor(blocks[:, t], device=DEV)
                f = env.add_new_blocks(b.float() if source == "f32" else b.contiguous(), active=act)
            f = _feat_np(f)
            after = _state(env)
            err = env.errors.cpu().numpy()
            for e in range(B):
                blk = seen_blocks[e, t]
                stepped = False
                if active[t, e]:
                    full = count[e] >= N_MAX
                    bad = bool((blk < 1).any())
                    if strategy == "MACS":                                        # its limit is part of the side check
                        bad = bad or _family_rejects(strategy, cs, blk)
                    elif not full and not bad:                                    # LB_GREEDY's is looked at last
                        bad = _family_rejects(strategy, cs, blk)
                    want_err[e] |= (2 if full else 0) | (4 if bad else 0)
                    stepped = not full and not bad
                if stepped:
                    rc, _ = orc[e].add_new_block(blk)
                    assert rc == 0 and orc[e].error == 0, (name, feat, t, e)
                    nstable[e] += int(orc[e].stable[count[e]])
                    count[e] += 1
                    assert np.array_equal(after["hm"][e], orc[e].heightmap.reshape(-1)), (name, feat, t, e)
                    assert np.array_equal(after["pos"][e], orc[e].positions), (name, feat, t, e)
                    assert np.array_equal(after["stable"][e], orc[e].stable.astype(np.uint8)), (name, feat, t, e)
                    assert list(after["cnt"][e]) == [orc[e].valid_size, orc[e].empty_size, nstable[e], count[e]], (name, feat, t, e)
                    assert _bits(after["ratio"][e]) == _bits(orc[e].calc_ratio()), (name, feat, t, e)
                else:                                                             # idle or refused: the state is untouched
                    for k in ("hm", "pos", "stable", "cnt"):
                        assert np.array_equal(after[k][e], before[k][e]), (name, feat, t, e, k)
                    assert _bits(after["ratio"][e]) == _bits(before["ratio"][e]), (name, feat, t, e)
                assert err[e] == want_err[e], (name, feat, t, e, err[e], want_err[e])   # exactly the expected bits
                assert np.array_equal(f[e], orc[e].get_heightmap().reshape(-1)), (name, feat, t, e)   # reported all the same
        assert want_err[0] & 2 and want_err[1] & 4                                # the plan met what it was made for
        assert np.array_equal(_feat_np(env.get_heightmaps()), np.stack([o.get_heightmap().reshape(-1) for o in orc]))


@pytest.mark.parametrize("cs,reward,strategy", [([66, 30], "mcs-soft", "MACS"), ([9, 9, 20], "C+P+S-mcs-soft", "MACS"),
                                                ([9, 8, 20], "C+P+S-lb-hard", "LB_GREEDY")],
                         ids=["k_macs2d_wave_transition", "k_macs3d_wave_transition", "k_big_transition"])
def test_fused_wave_transitions_file_the_gather(T, cs, reward, strategy):
    """the decoding step in one launch (fresh first step, calc_ratio on the last): decoder_static and the tour against
    the host-side gather, the episode against the oracle"""
    from tap_net_amd import pack, synth
    B, n, D = 5, 4, len(cs)
    static, dynamic = synth.rand_instances(B, n, D, seed=31)
    tape = synth.random_feasible_tape(static, dynamic, n, seed=32)
    env = T.BatchedContainer(B, cs, n, reward, "diff", packing_strategy=strategy, device=DEV)
    stp = pack.EpisodeStepper(static.to(DEV), dynamic.to(DEV), env, steps=n)
    st = static.numpy()
    bl = np.stack([st[np.arange(B), 1:, tape[:, t].numpy()] for t in range(n)], axis=1)
    want = O.run_episodes(O.make_desc(cs, n, reward, "diff", strategy), bl.astype(np.int32))
    assert want["nerr"] == 0
    for rep in range(2):                                                          # the second episode starts from a used blob
        stp.begin(static.to(DEV), dynamic.to(DEV))
        for t in range(n):
            stp.step(tape[:, t].to(DEV))
            assert np.array_equal(stp.decoder_static.cpu().numpy().reshape(B, D), bl[:, t]), (rep, t)
            assert np.array_equal(_feat_np(stp.decoder_dynamic), want["features"][:, t]), (rep, t)
        assert np.array_equal(stp.tour.cpu().numpy(), tape.numpy())
        env.check()
        assert np.array_equal(env.positions.cpu().numpy(), want["positions"])
        assert np.array_equal(env.stable.cpu().numpy().astype(np.uint8), want["stable"])
        assert np.array_equal(stp.ratio.cpu().numpy(), want["ratio"].astype(np.float32))
        assert np.array_equal(_bits(env.calc_ratios64().cpu().numpy()), _bits(want["ratio"]))


def test_fallback_kernels_take_the_same_cases():
    """k_big_step, k_macs2d_big_step, k_macs3d_big_step: the cases above once more with the wave kernels out of the way
    (TAP_NO_WAVE_KERNELS is read once per process), in a process of their own"""
    env = dict(os.environ, TAP_NO_WAVE_KERNELS="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_step_seam_vs_oracle or test_fused_wave_transitions"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    assert " passed" in p.stdout and "failed" not in p.stdout
