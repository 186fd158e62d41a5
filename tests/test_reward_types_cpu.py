"""The reference's legacy reward names (tests/reward_type_cases.py) on the CPU: tests/golden/reward_types.npz -- the
reference's tools.Container, calc_positions_lb_greedy and calc_positions_mcs under 'comp', 'soft', 'hard', 'pyrm',
'pyrm-soft', 'pyrm-hard', 'pyrm-soft-sum', 'pyrm-hard-sum', 'pyrm-soft-SUM', 'pyrm-hard-SUM' and 'CPS' -- pins the oracle
bit for bit; tap_env_desc_init gives every name the flags and the ratio mode the table states; and the inputs
tests/test_reward_types_gpu.py shares are strong enough that a kernel wrong on these names cannot pass: the placements
differ from the already-tested twin reward's, the ratio differs from (C + P + S) / 3, and no container raises."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
import oracle_lib as O
import ref_loader
import reward_type_cases as RC
from tap_net_amd import _lib

STRATEGY = {"LB_GREEDY": O.LB_GREEDY, "MACS": O.MACS, "LB": O.LB}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def rec():
    return G.load("reward_types.npz")


def test_fixture_lists_the_table(rec):
    assert [k.decode() for k in rec["traces"]] == [RC.trace_key(s, name) for s, name, _ in RC.trace_plan()]
    assert len(rec["list_status"]) == len(RC.list_plan())
    assert len(rec["list_ratio"]) == len(rec["list_scores"]) == len(rec["list_digest"]) == int((rec["list_status"] == 0).sum())
    plan = RC.trace_plan()
    for strategy in ("LB_GREEDY", "LB", "MACS"):
        for D in (2, 3):
            assert {name for s, name, _ in plan if s.strategy == strategy and s.D == D} >= set(RC.ALL), (strategy, D)
    wide = {(s.strategy, s.cs) for s, _, _ in plan}
    assert wide >= {("LB_GREEDY", (70, 60)), ("LB_GREEDY", (10, 10, 60)), ("MACS", (20, 60)), ("MACS", (70, 60)),
                    ("MACS", (10, 10, 40))}
    assert {f for _, _, f in plan} == set(RC.FEATURES)
    assert any(n == 0 for _, _, n, _, _, _ in RC.list_plan())
    assert os.path.getsize(os.path.join(G.GOLDEN, "reward_types.npz")) < 3 * os.path.getsize(os.path.join(G.GOLDEN, "window_forms.npz"))
    assert set(rec.files) == {"traces", "trace_digests", "trace_counters", "trace_offsets", "trace_ratio", "trace_cps",
                              "list_status", "list_ratio", "list_scores", "list_digest"}


@pytest.mark.parametrize("k", range(len(RC.trace_plan())), ids=[RC.trace_key(s, n) for s, n, _ in RC.trace_plan()])
def test_oracle_container_equals_the_reference(rec, k):
    """height-map, feature, positions / stable, valid_size and empty_size after every step; calc_ratio and calc_CPS at
    the end by their bit patterns"""
    shape, name, feat = RC.trace_plan()[k]
    B = RC.GOLDEN_B
    blocks = shape.blocks(B)
    want = rec["trace_digests"][rec["trace_offsets"][k]:rec["trace_offsets"][k + 1]]
    want_cnt = rec["trace_counters"][rec["trace_offsets"][k]:rec["trace_offsets"][k + 1]]
    assert want.shape == (shape.n, 3, RC.TRACE_DIGEST)
    envs = [O.Env(list(shape.cs), shape.n, name, feat, shape.strategy) for _ in range(B)]
    for t in range(shape.n):
        feats = []
        for b, e in enumerate(envs):
            rc, f = e.add_new_block(blocks[b, t])
            assert rc == 0 and e.error == 0
            feats.append(np.asarray(f).reshape(-1))
        hm = np.stack([e.heightmap.reshape(-1) for e in envs])
        pos = np.stack([e.positions[:t + 1] for e in envs])
        stb = np.stack([e.stable[:t + 1] for e in envs])
        where = "%s / %s step %d" % (shape.name, name, t)
        assert np.array_equal(RC.digest((hm, np.int32))[:RC.TRACE_DIGEST], want[t, 0]), "height-map, " + where
        assert np.array_equal(RC.digest((np.stack(feats), np.int32))[:RC.TRACE_DIGEST], want[t, 1]), "feature, " + where
        assert np.array_equal(RC.digest((pos, np.int32), (stb, np.uint8))[:RC.TRACE_DIGEST], want[t, 2]), "positions / stable, " + where
        assert [[e.valid_size, e.empty_size] for e in envs] == want_cnt[t].tolist(), "counters, " + where
    got = np.asarray([e.calc_ratio() for e in envs])
    assert np.array_equal(_bits(got), _bits(rec["trace_ratio"][k])), (got, rec["trace_ratio"][k])
    cps = np.zeros((B, 3), np.float64)
    for b, e in enumerate(envs):
        O.lib().orc_env_cps(e._h, cps[b].ctypes.data_as(C.c_void_p))
    assert np.array_equal(_bits(cps), _bits(rec["trace_cps"][k]))
    # and the formula of the table, from the reference's own C, P, S
    Cc, P, S = rec["trace_cps"][k].T
    assert np.array_equal(_bits(RC.formula(RC.RATIO_MODE[name], Cc, P, S)), _bits(rec["trace_ratio"][k]))


def test_oracle_episode_functions_equal_the_reference(rec):
    """calc_positions_lb_greedy / calc_positions_mcs: positions, stable flags, the fp64 ratio by its bits and the five
    scores wherever the reference returns; and the reference returns exactly for the names each function has a formula
    for -- it raises UnboundLocalError for the rest (the oracle and the product's kernels score those C + P + S, which
    nothing here pins) and IndexError for an empty list"""
    status = [RC.LIST_STATUS[v] for v in rec["list_status"]]
    seen = set()
    ok = -1
    for i, (fn, cs, n, side, k, name) in enumerate(RC.list_plan()):
        scored = RC.LBG_SCORED if fn.endswith("greedy") else RC.MCS_SCORED
        want = "IndexError" if n == 0 else "ok" if name in scored else "UnboundLocalError"
        assert status[i] == want, (fn, cs, n, name, status[i])
        if status[i] != "ok":
            continue
        ok += 1
        blocks = RC.golden_list(cs, n, side, k)
        rc, pos, stb, ratio, scores = getattr(O, fn)(blocks, list(cs), name)
        assert rc == 0
        where = "%s %s n=%d list %d %s" % (fn, cs, n, k, name)
        assert np.array_equal(RC.digest((pos, np.int32), (stb, np.uint8)), rec["list_digest"][ok]), where
        assert _bits(ratio) == _bits(rec["list_ratio"][ok]), (where, ratio, rec["list_ratio"][ok])
        assert scores.tolist() == rec["list_scores"][ok].tolist(), where
        seen.add((fn, name))
    assert seen == {("calc_positions_lb_greedy", "C+P-lb-soft")} | {("calc_positions_mcs", n) for n in RC.ALL}


def test_generator_reproduces_the_fixture(tmp_path):
    if not ref_loader.available():
        pytest.skip("the reference checkout is not present")
    out = str(tmp_path / "reward_types.npz")
    subprocess.check_call([sys.executable, os.path.join(G.GOLDEN, "make_golden_reward_types.py"), out])
    new, old = np.load(out, allow_pickle=False), G.load("reward_types.npz")
    assert set(new.files) == set(old.files)
    for k in old.files:                                               # (compressed: the arrays, not the zip's bytes)
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), k


# ---- the descriptor --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["LB_GREEDY", "LB", "MACS"])
@pytest.mark.parametrize("name", RC.ALL + ["C+P-lb-soft"])
def test_descriptor_carries_what_the_table_states(name, strategy):
    hard, p, s, mode = RC.NAMES.get(name, (0, 1, 0, "R_CP_HALF"))
    flags = hard * O.F_HARD | p * O.F_USE_P | s * O.F_USE_S                 # no name here holds 'mcs': no ZERO / TIE bit
    for cs, feat in (([5, 50], "diff"), ([5, 6, 50], "zero"), ([70, 60], "full")):
        d = _lib.make_desc(7, cs, 10, name, feat, strategy)
        o = O.make_desc(cs, 10, name, feat, strategy)
        for f in ("D", "W", "L", "H", "n_max", "strategy", "flags", "ratio_mode", "feature"):
            assert getattr(d, f) == getattr(o, f), (name, strategy, f)
        assert (d.strategy, d.flags, d.ratio_mode, d.feature) == (STRATEGY[strategy], flags, getattr(O, mode), O.FEAT[feat])


def test_the_table_names_every_class():
    assert len(RC.ALL) == 11 and set(RC.REPRESENTATIVES) <= set(RC.ALL) and set(RC.RATIO_NAMES) - {"C+P-lb-soft"} <= set(RC.ALL)
    assert {RC.NAMES[n][:3] for n in RC.REPRESENTATIVES} == {v[:3] for v in RC.NAMES.values()}
    assert {RC.RATIO_MODE[n] for n in RC.RATIO_NAMES} == {"R_C", "R_CxS", "R_CP", "R_CPxS", "R_CPS", "R_2CPS", "R_CxPxS", "R_CP_HALF"}
    steps = RC.step_cases()
    for s in RC.BASE:
        assert {n for sh, n, _ in steps if sh == s} == set(RC.ALL)
    for s in RC.FAMILIES:
        assert {n for sh, n, _ in steps if sh == s} == set(RC.REPRESENTATIVES)
    for strategy in ("LB_GREEDY", "LB", "MACS"):
        assert {f for sh, _, f in steps if sh.strategy == strategy} == set(RC.FEATURES)
    for s in RC.STEP_SHAPES:
        assert 65 <= s.B <= 300 and s.B % 8 != 0


# ---- coverage: what the shared inputs must do, computed with the oracle alone ------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_run(shape, name):
    return RC.run(O, shape, name, want_features=False)


@functools.lru_cache(maxsize=None)
def _fused_run(shape, name):
    c = RC.fused_case(shape, name)
    blocks = RC.fused_blocks(c, RC.fused_build(c))
    return O.run_episodes(O.make_desc(list(c.cs), c.n, name, "diff", c.strategy), blocks, want_features=False)


def _moved(run, twin):
    assert run["nerr"] == 0 and twin["nerr"] == 0
    return float((run["positions"] != twin["positions"]).any(axis=(1, 2)).mean())


@pytest.mark.parametrize("shape", RC.STEP_SHAPES, ids=lambda s: s.name)
def test_placements_move_on_the_step_shapes(shape):
    """for every representative but 'CPS' (which sets its twin's flags) at least a quarter of the containers get
    positions other than the twin reward's on the same blocks"""
    for name in RC.REPRESENTATIVES:
        share = _moved(_step_run(shape, name), _step_run(shape, RC.twin(name)))
        if name == "CPS":
            assert share == 0
        else:
            assert share >= 0.25, "%s / %s: %.2f of the containers differ from %s" % (shape.name, name, share, RC.twin(name))


@pytest.mark.parametrize("shape", RC.FUSED_SHAPES, ids=lambda s: "%s-%s" % (s[0], "x".join(map(str, s[1]))))
def test_placements_move_on_the_fused_shapes(shape):
    for name in RC.REPRESENTATIVES:
        share = _moved(_fused_run(shape, name), _fused_run(shape, RC.twin(name)))
        assert share == 0 if name == "CPS" else share >= 0.25, (shape, name, share)


def _formula_shows(name, ratio, cps, where):
    """the share of containers whose ratio is not (C + P + S) / 3 of the same C, P, S.  'pyrm-soft-sum' IS that
    formula (tools.py:3929): its share is zero by definition, and what tells it from its neighbours is its flag class"""
    base = (cps[:, 0] + cps[:, 1] + cps[:, 2]) / 3
    share = float((_bits(ratio) != _bits(base)).mean())
    if RC.RATIO_MODE[name] == "R_CPS":
        assert share == 0, where
    else:
        assert share >= 0.9, "%s: only %.2f of the ratios differ from (C + P + S) / 3" % (where, share)


@pytest.mark.parametrize("name", RC.RATIO_NAMES)
def test_the_ratio_formula_shows(name):
    for shape in RC.BASE:
        run = _step_run(shape, name)
        assert run["nerr"] == 0
        _formula_shows(name, run["ratio"], run["cps"], "%s / %s" % (shape.name, name))
        assert np.array_equal(_bits(RC.formula(RC.RATIO_MODE[name], *run["cps"].T)), _bits(run["ratio"]))
    for shape in RC.FUSED_SHAPES:
        run = _fused_run(shape, name)
        assert run["nerr"] == 0
        _formula_shows(name, run["ratio"], run["cps"], "fused %s / %s" % (shape, name))


def test_no_case_is_dropped():
    """nerr == 0 for every case the GPU file runs: nothing is masked out as 'the reference raises'"""
    for shape, name, feat in RC.step_cases():
        assert _step_run(shape, name)["nerr"] == 0, (shape.name, name)
    for shape in RC.FUSED_SHAPES:
        for name in RC.fused_names():
            assert _fused_run(shape, name)["nerr"] == 0, (shape, name)
    for shape in RC.EPISODE_SHAPES:
        D, W, H, n, B, strategy = shape[:6]
        static, tour, blocks = RC.episode_inputs(shape)
        cs = [W, H] if D == 2 else [W, W, H]
        strat = "LB_GREEDY" if strategy == "LB_GREEDY" else "MACS"
        names = [v for v in RC.REPRESENTATIVES if v in RC.EPISODE_NAMES and v != "CPS"]
        assert names == ["comp", "hard", "pyrm-soft-SUM"]
        for name in names:                                              # every representative the episodes run
            run = O.run_episodes(O.make_desc(cs, n, name, "full", strat), blocks, want_features=False)
            twin = O.run_episodes(O.make_desc(cs, n, RC.twin(name), "full", strat), blocks, want_features=False)
            assert _moved(run, twin) >= 0.25, (RC.episode_id(shape), name, _moved(run, twin))
        for name in RC.RATIO_NAMES:
            if strategy != "LB_GREEDY" and name not in RC.MCS_SCORED:
                continue
            ratio, scores, errs = O.render_scores(static, tour, name, "bot", True, W, H, strategy, initial_container_height=H)
            assert not errs.any(), (D, W, strategy, name)
            if strategy != "LB_GREEDY" and RC.RATIO_MODE[name] != "R_CPS":      # calc_positions_mcs: the formula, not over 3
                valid, box, empty, nst = (scores[:, k] for k in range(4))
                base = (valid / box + valid / (empty + valid)) + nst / n
                assert (_bits(ratio) != _bits(base)).mean() >= 0.9, (D, W, strategy, name)
