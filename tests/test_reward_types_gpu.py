"""The reference's legacy reward names -- 'comp', 'soft', 'hard', 'pyrm', 'pyrm-soft', 'pyrm-hard', 'pyrm-soft-sum',
'pyrm-hard-sum', 'pyrm-soft-SUM', 'pyrm-hard-SUM', 'CPS' (tests/reward_type_cases.py) -- through every placement kernel
on the GPU: stand-alone steps, fused steps, whole episodes, rolling steps, trial scores and the tools.Container facade.

Every comparison is against the CPU oracle, which tests/test_reward_types_cpu.py pins to the reference on these names
(tests/golden/reward_types.npz), bit for bit: integers exactly, fp64 by bit pattern, fp32 against the oracle's value cast
to fp32.  The same CPU file asserts that the shared inputs are strong enough: the placements differ from the twin
reward's in at least a quarter of the containers, and the ratio from (C + P + S) / 3 in at least nine of ten.  With P
and S off most candidates of a step tie, so these names are the sharpest test the suite has of the first-come order of
every cross-lane argmax."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import best_order_cases as BC
import golden_util as G
import oracle_lib as O
import reward_type_cases as RC
import stream_cases as S
import window_forms as WF

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NO_WAVE = bool(os.environ.get("TAP_NO_WAVE_KERNELS"))


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _eq(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r != %r" % (what, len(bad), bad[0].tolist(), got[tuple(bad[0])],
                                                                         want[tuple(bad[0])])


def _eq64(got, want, what):
    """fp64 by bit pattern"""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == np.float64, what
    _eq(_bits(got), _bits(want), what)


# ---- a. stand-alone steps ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_ref(shape, name, feat):
    """the oracle's episodes with every intermediate state, computed once and read-only"""
    blocks = shape.blocks()
    ref = RC.run(O, shape, name, feat, nthreads=8)
    # the counters after every step: the oracle's container, one env at a time
    cnt = np.zeros((shape.B, shape.n, 3), np.int64)               # valid_size, empty_size, stable_num (np.sum(stable))
    for b in range(shape.B):
        e = O.Env(list(shape.cs), shape.n, name, feat, shape.strategy)
        for t in range(shape.n):
            e.add_new_block(blocks[b, t])
            cnt[b, t] = e.valid_size, e.empty_size, int(e.stable[:t + 1].sum())
    assert np.array_equal(cnt[:, -1, :2], ref["counters"][:, :2]) and np.array_equal(cnt[:, -1, 2], ref["stable"].sum(axis=1))
    assert (ref["counters"][:, 2] == shape.n).all()                # (the oracle's third counter is the block count)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return blocks, ref, cnt


@pytest.mark.parametrize("shape,name,feat", RC.step_cases(), ids=lambda v: v.name if isinstance(v, RC.Shape) else v)
def test_steps_against_the_oracle(T, shape, name, feat):
    """BatchedContainer.add_new_blocks: feature, height-map and counters after every step; positions, stable flags,
    calc_ratios64, calc_ratios and calc_CPS at the end"""
    blocks, ref, cnt = _step_ref(shape, name, feat)
    assert ref["nerr"] == 0
    B, n = shape.B, shape.n
    where = "%s / %s / %s" % (shape.name, name, feat)
    env = T.BatchedContainer(B, list(shape.cs), n, name, feat, packing_strategy=shape.strategy, device=DEV)
    blk = torch.as_tensor(blocks.astype(np.float32), device=DEV)
    for t in range(n):
        f = env.add_new_blocks(blk[:, t].contiguous())
        _eq(f.reshape(B, -1).to(torch.int64), ref["features"][:, t].astype(np.int64), "feature, %s step %d" % (where, t))
        _eq(env.heightmap.reshape(B, -1), ref["heightmaps"][:, t], "height-map, %s step %d" % (where, t))
        c = env.counters.cpu().numpy()
        _eq(c[:, :3], cnt[:, t], "valid / empty size and stable count, %s step %d" % (where, t))
        assert (c[:, 3] == t + 1).all(), where
    env.check()
    _eq(env.counters.cpu().numpy()[:, :3], cnt[:, -1], "counters, " + where)
    _eq(env.positions, ref["positions"], "positions, " + where)
    _eq(env.stable.to(torch.uint8), ref["stable"], "stable, " + where)
    _eq64(env.calc_ratios64(), ref["ratio"], "calc_ratios64, " + where)
    _eq(env.calc_ratios(), ref["ratio"].astype(np.float32), "calc_ratios, " + where)
    _eq64(env.calc_CPS(), ref["cps"], "calc_CPS, " + where)
    assert np.array_equal(_bits(RC.formula(RC.RATIO_MODE[name], *ref["cps"].T)), _bits(ref["ratio"])), where


# ---- b. fused steps ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fused_ref(shape, name):
    c = RC.fused_case(shape, name)
    inp = RC.fused_build(c)
    return c, inp, WF.oracle_run(O, c, inp)


def _expand(bits, B, rows, nR):
    words = bits.view(B, -1, nR)
    r = torch.arange(rows, device=bits.device)
    return ((words[:, (r // 64)] >> (r % 64).view(1, -1, 1)) & 1).to(torch.float32)


def _check_fused_step(c, run, t, where, dyn, bits, cur, mask, feat):
    where = "%s step %d" % (where, t)
    _eq(dyn, run["dynamic"][t], "dynamic, " + where)
    if bits is not None:
        _eq(_expand(bits, c.B, c.rows, c.nR), run["dynamic"][t], "bit shadow, " + where)
    _eq(cur, run["current"][t], "current_mask, " + where)
    _eq(mask, run["mask"][t], "mask, " + where)
    _eq(feat.reshape(c.B, -1).to(torch.int64), run["episode"]["features"][:, t].astype(np.int64), "feature, " + where)


def _check_fused_end(c, run, env, ratio, where):
    ep = run["episode"]
    assert ep["nerr"] == 0
    _eq(env.positions, ep["positions"], "positions, " + where)
    _eq(env.stable.to(torch.uint8), ep["stable"], "stable, " + where)
    _eq(env.heightmap.reshape(c.B, -1), ep["heightmaps"][:, -1], "height-map, " + where)
    _eq(env.errors, np.zeros(c.B, np.int32), "error flags, " + where)
    assert ratio.dtype == torch.float32
    _eq(ratio, ep["ratio"].astype(np.float32), "the launch's fp32 ratio, " + where)
    _eq64(env.calc_ratios64(), ep["ratio"], "calc_ratios64, " + where)


_FUSED = [(s, n) for s in RC.FUSED_SHAPES for n in RC.fused_names()]
_fused_id = lambda v: v if isinstance(v, str) else "%s-%s" % (v[0], "x".join(map(str, v[1])))     # noqa: E731


@pytest.mark.parametrize("shape,name", _FUSED, ids=_fused_id)
def test_env_transition_against_the_oracle(T, shape, name):
    """pack.EnvTransition: mask, dynamic, its bit shadow and the placement after every step, the ratio of the last
    launch; the launch record names the launcher the shape was chosen for"""
    from tap_net_amd import pack
    c, inp, run = _fused_ref(shape, name)
    st, dy, tape = (torch.tensor(inp[k], device=DEV) for k in ("static", "dynamic", "tape"))
    where = c.name + " EnvTransition"
    env = T.BatchedContainer(c.B, list(c.cs), c.n, name, "diff", packing_strategy=c.strategy, device=DEV)
    T._lib.variant_hits_reset(DEV)
    et = pack.EnvTransition(st, dy, env, c.input_type, c.allow_rot)
    assert et.bits is not None, where
    _eq(et.current_mask, run["initial"], "initial current_mask, " + where)
    ratio = None
    for t in range(c.nsteps):
        d, cur, mask, feat, ratio = et.step(tape[:, t], fresh=(t == 0), want_ratio=(t == c.nsteps - 1))
        _check_fused_step(c, run, t, where, d, et.bits, cur, mask, feat)
    _check_fused_end(c, run, env, ratio, where)
    WF.check_keys(c, T._lib.variant_keys(DEV))


@pytest.mark.parametrize("shape,name", _FUSED, ids=_fused_id)
def test_episode_stepper_against_the_oracle(T, shape, name):
    from tap_net_amd import pack
    c, inp, run = _fused_ref(shape, name)
    st, dy, tape = (torch.tensor(inp[k], device=DEV) for k in ("static", "dynamic", "tape"))
    where = c.name + " EpisodeStepper"
    env = T.BatchedContainer(c.B, list(c.cs), c.n, name, "diff", packing_strategy=c.strategy, device=DEV)
    sp = pack.EpisodeStepper(st, dy, env, input_type=c.input_type, allow_rot=c.allow_rot, steps=c.nsteps)
    T._lib.variant_hits_reset(DEV)
    sp.begin(st, dy, initial_mask=True)
    _eq(sp.current_mask, run["initial"], "initial current_mask, " + where)
    for t in range(c.nsteps):
        sp.step(tape[:, t].contiguous())
        _check_fused_step(c, run, t, where, sp.dynamic, sp.dynamic_bits, sp.current_mask, sp.mask, sp.decoder_dynamic)
    torch.cuda.synchronize()
    _check_fused_end(c, run, env, sp.ratio, where)
    _eq(sp.tour, inp["tape"], "tour, " + where)
    _eq(dy, inp["dynamic"], "the caller's dynamic, " + where)
    WF.check_keys(c, T._lib.variant_keys(DEV))
    sp.check()


# ---- c. whole episodes -----------------------------------------------------------------------------------------------------
EPISODE_NAMES = RC.EPISODE_NAMES
_WAVE = [s for s in RC.EPISODE_SHAPES if s[1] > 8]
_EPISODE_KINDS = {16, 17, 18, 23, 24}                            # tapenv.h: the launch record's whole-episode kernels


@pytest.fixture
def stepped(monkeypatch):
    """counts the stand-alone placement launches the stepped forms of the whole-episode functions are made of
    (pack._stepped_scores, pack.reward's and generate.pack_blocks' fallbacks); ``stepped.expect(shape, what)``: none
    where a one-launch kernel answers, n under TAP_NO_WAVE_KERNELS on a container above the lane kernels"""
    from tap_net_amd.env import BatchedContainer

    class Count(object):
        calls = 0

        def expect(self, shape, what):
            want = shape[3] if (NO_WAVE and shape[1] > 8) else 0
            assert self.calls == want, "%s: %d stepped placement launches, expected %d" % (what, self.calls, want)
            self.calls = 0

    count = Count()
    for meth in ("add_new_blocks", "add_new_blocks_gather"):
        real = getattr(BatchedContainer, meth)

        def wrapped(self, *a, _real=real, **kw):
            count.calls += 1
            return _real(self, *a, **kw)

        monkeypatch.setattr(BatchedContainer, meth, wrapped)
    return count


@functools.lru_cache(maxsize=None)
def _episode_inputs(shape):
    return RC.episode_inputs(shape)


@pytest.mark.parametrize("name", EPISODE_NAMES)
@pytest.mark.parametrize("shape", RC.EPISODE_SHAPES, ids=RC.episode_id)
def test_whole_episodes_against_the_oracle(T, stepped, shape, name):
    """LB_GREEDY: pack.reward and generate.pack_blocks score C + P + S under every name, pack.episode_scores where
    tools.calc_positions_lb_greedy has a formula and its UnboundLocalError elsewhere.  MACS / MUL: pack.episode_scores
    and tap_pack_blocks by calc_positions_mcs' table (tools.py:3281-3309).  One launch each: no stepped placement runs
    and the launch record holds the episode kernel of the name's flag class (the wave episode of big.hip keeps no
    record); under TAP_NO_WAVE_KERNELS the containers above the lane kernels take n stepped launches and no episode
    kernel."""
    from tap_net_amd import _lib, generate, pack
    D, W, H, n, B, strategy = shape[:6]
    static, tour, blocks = _episode_inputs(shape)
    cs = [W, H] if D == 2 else [W, W, H]
    st, tr = torch.as_tensor(static, device=DEV), torch.as_tensor(tour, device=DEV)
    where = "%s / %s" % (shape, name)
    hard = name.endswith("hard")
    _lib.variant_hits_reset(DEV)
    if strategy == "LB_GREEDY":
        nerr, want = O.reward(static, tour, name, W, H)
        assert nerr == 0
        _eq(pack.reward(st, tr, name, "bot", True, W, H), want, "pack.reward, " + where)
        stepped.expect(shape, "pack.reward, " + where)
        ref = O.run_episodes(O.make_desc(cs, n, name, "full", "LB_GREEDY"), blocks, want_features=False, want_heightmaps=False)
        pos, stb, rew = generate.pack_blocks(torch.as_tensor(blocks, device=DEV), cs, name)
        _eq(pos, ref["positions"], "pack_blocks positions, " + where)
        _eq(stb.to(torch.uint8), ref["stable"], "pack_blocks stable, " + where)
        _eq(rew, want, "pack_blocks reward, " + where)
        stepped.expect(shape, "pack_blocks, " + where)
        if NO_WAVE and W > 8:
            assert not {k[0] for k in _lib.variant_keys(DEV)} & _EPISODE_KINDS, (where, sorted(_lib.variant_keys(DEV)))
        if W <= 8 and not NO_WAVE:
            G_ = S.group_size(WF.Case("bot", D, tuple(cs), n))
            assert (16, D, G_, 0 if hard else 1, 0, 0, 0) in _lib.variant_keys(DEV), (where, sorted(_lib.variant_keys(DEV)))
        if name not in RC.LBG_SCORED:
            with pytest.raises(UnboundLocalError):
                pack.episode_scores(st, tr, name, "bot", True, cs, "LB_GREEDY")
            return
    elif name not in RC.MCS_SCORED:
        with pytest.raises(UnboundLocalError):
            pack.episode_scores(st, tr, name, "bot", True, cs, strategy)
        return
    want_r, want_s, errs = O.render_scores(static, tour, name, "bot", True, W, H, strategy, initial_container_height=H)
    assert not errs.any()
    _lib.variant_hits_reset(DEV)
    r, sc = pack.episode_scores(st, tr, name, "bot", True, cs, strategy)
    _eq64(r, want_r, "episode_scores ratio, " + where)
    _eq(sc.double(), want_s, "episode_scores scores, " + where)
    stepped.expect(shape, "episode_scores, " + where)
    if NO_WAVE and W > 8:
        assert not {k[0] for k in _lib.variant_keys(DEV)} & _EPISODE_KINDS, (where, sorted(_lib.variant_keys(DEV)))
    if strategy != "LB_GREEDY":
        if not NO_WAVE:
            kind = {(2, False): 17, (3, False): 18, (2, True): 23, (3, True): 24}[(D, W > 8)]
            assert kind in {k[0] for k in _lib.variant_keys(DEV)}, (where, sorted(_lib.variant_keys(DEV)))
        ref = O.run_episodes(O.make_desc(cs, n, name, "full", "MACS"), blocks, want_features=False, want_heightmaps=False)
        desc = _lib.make_desc(B, cs, n, name, "full", "MACS")
        blk = torch.as_tensor(blocks, device=DEV)
        pos = torch.zeros(B, n, D, dtype=torch.int32, device=DEV)
        stab = torch.zeros(B, n, dtype=torch.uint8, device=DEV)
        s64 = torch.zeros(B, dtype=torch.float64, device=DEV)
        c = _lib.ctx(DEV)
        status = _lib.lib().tap_pack_blocks(c, C.byref(desc), B, n, _lib.ptr(blk), None, _lib.ptr(pos), _lib.ptr(stab),
                                            _lib.ptr(s64), _lib.stream_of(torch.device(DEV)))
        if not (NO_WAVE and status == _lib.TAP_E_UNSUPPORTED):    # (no stepped form behind the C entry point itself)
            _lib.check(status, c)
            _eq(pos, ref["positions"], "tap_pack_blocks positions, " + where)
            _eq(stab, ref["stable"], "tap_pack_blocks stable, " + where)
            _eq64(s64, want_r, "tap_pack_blocks score, " + where)


@pytest.mark.parametrize("strategy", ["LB_GREEDY", "MACS"])
def test_empty_target_list(T, strategy):
    """the two-container input types: a container whose list is empty scores zeros (pack.py:760-769) under every name"""
    from tap_net_amd import pack
    D, W, H, n, B = 2, 5, 50, 8, 65
    static, tour, _ = RC.episode_inputs((D, W, H, n, B, strategy, (1, 4), 4))
    ids = np.zeros((B, 1, static.shape[2]), np.float32)
    ids[1::2] = np.tile((np.arange(n) % 2).astype(np.float32), 2)             # odd envs: both lists; even envs: list 1 empty
    static = np.concatenate((static, ids), axis=1)
    st, tr = torch.as_tensor(static, device=DEV), torch.as_tensor(tour, device=DEV)
    for name in RC.RATIO_NAMES:
        if name not in (RC.LBG_SCORED if strategy == "LB_GREEDY" else RC.MCS_SCORED):
            continue
        want_r, want_s, errs = O.render_scores(static, tour, name, "mul", True, W, H, strategy, initial_container_height=H)
        assert not errs.any()
        ra, sa = pack.episode_scores(st, tr, name, "mul", True, [W, H], strategy, target=0)
        rb, sb = pack.episode_scores(st, tr, name, "mul", True, [W, H], strategy, target=1)
        assert bool((rb[0::2] == 0).all()) and bool((sb[0::2] == 0).all()), name
        _eq64((ra + rb) / 2, want_r, "ratio, " + name)
        _eq((sa.double() + sb.double()) / 2, want_s, "scores, " + name)


def test_whole_episodes_without_the_wave_kernels():
    """pack._stepped_scores and the stepped pack_blocks / reward: the wave-episode shapes again under
    TAP_NO_WAVE_KERNELS (read once per process), in a process of their own"""
    env = dict(os.environ, TAP_NO_WAVE_KERNELS="1")
    wave = " or ".join(RC.episode_id(s) for s in _WAVE)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_whole_episodes_against_the_oracle and (%s)" % wave],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    assert "%d passed" % (len(_WAVE) * len(EPISODE_NAMES)) in p.stdout, p.stdout[-500:]


# ---- d. rolling steps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_rolling_steps_with_p_and_s_off(T, D):
    """run_rolling_episode (the fused rolling step) under 'comp' -- k_rolling_step_soft -- and 'hard' -- the hard
    instantiation --: final packing and reward against the oracle container, and the launch record"""
    from tap_net_amd import generate as gen
    N, child, B, W = 24, 8, 65, 5
    init = [7, 120] if D == 2 else [7, 7, 120]
    static, dynamic, blocks, positions = gen.generate_instances(B, N, D, init[0], init[-1], 1, (1, 5), seed=11,
                                                                device=DEV, return_aux=True)
    H = 4 * N + 10
    cs = [W, H] if D == 2 else [W, W, H]
    moved = {}
    for name in ("comp", "hard"):
        g = torch.Generator(device=DEV)
        g.manual_seed(9)
        seen = {}

        def policy(step, static, dynamic, current_mask, **_):
            seen[step] = static.cpu().numpy()
            return torch.multinomial(current_mask, 1, generator=g).squeeze(1)

        T._lib.variant_hits_reset(DEV)
        out = T.run_rolling_episode(blocks, positions, init, policy, W, H, child_graph_size=child, reward_type=name)
        assert out["env"].fused_ok
        out["env"].check(); out["windows"].check()
        keys = {k for k in T._lib.variant_keys(DEV) if k[0] == 19}
        assert keys and {k[3] for k in keys} == {0 if name == "hard" else 1}, (name, sorted(keys))
        tour = out["tour_idx"].cpu().numpy()
        pos = out["env"].positions.cpu().numpy()
        rew = out["reward"].cpu().numpy()
        differ = 0
        for b in range(B):
            e, tw = O.Env(cs, N, name, "diff"), O.Env(cs, N, RC.twin(name), "diff")
            for t in range(N):
                blk = seen[min(t, N - child)][b][1:, int(tour[b, t])]
                rc, _ = e.add_new_block(blk)
                assert rc == 0
                tw.add_new_block(blk)
            assert np.array_equal(e.positions, pos[b]), (name, b)
            assert np.float32(e.calc_ratio()) == -rew[b], (name, b)
            differ += int(not np.array_equal(e.positions, tw.positions))
        moved[name] = differ / B
    assert min(moved.values()) >= 0.25, moved                     # the names change what these episodes place


# ---- e. trial scores -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.RATIO_NAMES)
@pytest.mark.parametrize("D,cs", [(2, [5, 50]), (3, [5, 5, 50])], ids=["5", "5x5"])
def test_trial_scores_against_an_oracle_replay(T, D, cs, name):
    """BatchedContainer.trial_scores mid-episode: the fp64 score of every selectable column by its bits, and the first
    column holding the row's maximum.  Under 'comp' most columns tie."""
    from tap_net_amd import pack, synth
    B, n = 67, 10
    static, dynamic = synth.rand_instances(B, n, D, seed=31 + D)
    static[:, 1:, :] = static[:, 1:, :].clamp(max=4.0)
    static = static.contiguous()
    tape = synth.random_feasible_tape(static, dynamic, n, seed=32 + D)
    st, dy = static.to(DEV), dynamic.to(DEV)
    st_np = static.numpy()
    env = T.BatchedContainer(B, cs, n, name, "full", device=DEV)
    masks = pack.MaskStepper(st, dy)
    committed = [[] for _ in range(B)]
    tied = rows = 0
    for t in range(6):
        if t in (0, 2, 5):
            cur = masks.current_mask
            m = cur.cpu().numpy()
            want = np.full(m.shape, -np.inf)
            for b in range(B):
                for col in np.flatnonzero(m[b]):
                    want[b, col] = BC.trial_score(cs, n, name, committed[b], st_np[b, 1:, col].astype(np.int32))
            before = env._state.clone()
            scores, best = env.trial_scores(st, cur)
            _eq64(scores, want, "trial scores, %s step %d" % (name, t))
            _eq(best, np.argmax(want, axis=1), "first maximum, %s step %d" % (name, t))
            assert torch.equal(env._state, before), "trial_scores wrote to the state blob"
            live = want.max(axis=1) > -np.inf
            rows += int(live.sum())
            tied += int(((want == want.max(axis=1, keepdims=True)).sum(axis=1) > 1)[live].sum())
        ptr = tape[:, t].to(DEV)
        for b in range(B):
            committed[b].append(st_np[b, 1:, int(tape[b, t])].astype(np.int32))
        masks.step(ptr)
        env.add_new_blocks_gather(st, ptr, want_feature=False)
    env.check()
    if name == "comp":                                            # the bar tests/test_trial_scores_gpu.py sets its tie inputs
        assert tied * 4 >= rows, "only %d of %d rows have a tied maximum under 'comp'" % (tied, rows)


# ---- f. the facade ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["comp", "pyrm-hard-SUM"])
def test_container_facade_gives_the_reference_s_ratio(T, name):
    """tools.Container over the fixture's blocks: calc_ratio() is the value the reference returned"""
    rec = G.load("reward_types.npz")
    plan = RC.trace_plan()
    for k, (shape, nm, feat) in enumerate(plan):
        if nm != name or shape not in RC.GOLDEN_TRACES[:6]:
            continue
        blocks = shape.blocks(RC.GOLDEN_B)
        for b in range(RC.GOLDEN_B):
            c = T.Container(list(shape.cs), shape.n, name, feat, packing_strategy=shape.strategy, device=DEV)
            for t in range(shape.n):
                c.add_new_block(blocks[b, t].astype(np.float32), False)
            got = c.calc_ratio()
            assert _bits(got) == _bits(rec["trace_ratio"][k, b]), (shape.name, name, b, got, rec["trace_ratio"][k, b])
            assert [c.valid_size, c.empty_size] == rec["trace_counters"][rec["trace_offsets"][k + 1] - 1, b].tolist()
