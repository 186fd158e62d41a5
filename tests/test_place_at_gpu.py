"""The pack-net placement on the MI355X (place_at.hip: k_place_at): every integer output bit-exact against the numpy
restatement (tests/place_at_model.py), which tests/test_place_at_cpu.py pins to the reference's traces."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import place_at_model as M
import tap_net_amd as T
from tap_net_amd import _lib, synth
from tap_net_amd.env import lockstep_scope

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "place_at.npz"))
CASES = [str(c) for c in G["cases"]]
RT = 'C+P+S-SL-soft'


def _place_at_launches():
    return {k: v for k, v in _lib.variant_hits(DEV).items() if k[0] == _lib.TAP_HIT_PLACE_AT}


def _compare(env, m, t=None, feat=None, pnet=None, form=None):
    hm, pos, st, cnt = env._export(True, True, True, True)
    assert np.array_equal(hm.cpu().numpy(), m.hm)
    assert np.array_equal(cnt.cpu().numpy(), m.counters())
    assert np.array_equal(pos.cpu().numpy(), m.positions)
    assert np.array_equal(st.cpu().numpy(), m.stable)
    assert np.array_equal(env.errors.cpu().numpy(), m.err)
    if feat is not None:
        assert np.array_equal(feat.cpu().numpy().reshape(m.B, -1).astype(np.int64), M.feature(m.hm, t))
    if pnet is not None:
        assert np.array_equal(pnet.cpu().numpy().reshape(m.B, -1).astype(np.int64), M.pnet_input(m.hm, form))


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("c_")])
def test_fixture_container_batched(name):
    W, H = (int(v) for v in G[name + "_cs"])
    t = name.rsplit("_", 1)[1]
    blocks, xs = G[name + "_blocks"], G[name + "_x"]
    n = len(xs)
    _lib.variant_hits_reset(DEV)
    env = T.BatchedContainer(1, [W, H], n, RT, t, device=DEV, place_at='container')
    for i in range(n):
        f = env.add_new_blocks_at(torch.as_tensor(blocks[i:i + 1]), torch.as_tensor(xs[i:i + 1]))
        assert np.array_equal(f.cpu().numpy().reshape(-1).astype(np.int64), G[name + "_feature"][i])
        assert env.counters[0, 0].item() == G[name + "_valid"][i] and env.counters[0, 1].item() == G[name + "_empty"][i]
        assert env.calc_ratios64()[0].item() == G[name + "_ratio"][i]
    assert np.array_equal(env.positions[0].cpu().numpy(), G[name + "_positions"])
    assert np.array_equal(env.stable[0].cpu().numpy().astype(np.uint8), G[name + "_stable"])
    env.check()
    assert _place_at_launches()


@pytest.mark.parametrize("pooled", [False, True])
def test_fixture_container_facade(pooled):
    names = [c for c in CASES if c.startswith("c_w5_") or c.startswith("c_w31_")]
    for name in names:
        W, H = (int(v) for v in G[name + "_cs"])
        t = name.rsplit("_", 1)[1]
        blocks, xs = G[name + "_blocks"], G[name + "_x"]
        n = len(xs)
        B = 6 if pooled else 1
        if pooled:
            with lockstep_scope():
                cs = [T.tools.Container([W, H], n, RT, t, device=DEV) for _ in range(B)]
                for i in range(n):
                    hms = [c.heightmap for c in cs]                      # DRL_L reads every height-map first
                    assert np.array_equal(hms[0], G[name + "_hm"][i - 1] if i else np.zeros(W, np.int64))
                    x = torch.full((B,), int(xs[i]), dtype=torch.int64, device=DEV)
                    rows = [c.add_new_block_at(blocks[i].astype(np.float32), x[b]) for b, c in enumerate(cs)]
                    for r in rows:
                        assert np.array_equal(np.asarray(r).reshape(-1), G[name + "_feature"][i])
        else:
            cs = [T.tools.Container([W, H], n, RT, t, device=DEV)]
            for i in range(n):
                f = cs[0].add_new_block_at(blocks[i].astype(np.float32), int(xs[i]))
                assert np.array_equal(np.asarray(f).reshape(-1), G[name + "_feature"][i])
        for c in cs:
            assert np.array_equal(c.positions, G[name + "_positions"])
            assert c.stable == [bool(v) for v in G[name + "_stable"]]
            assert c.valid_size == G[name + "_valid"][-1] and c.empty_size == G[name + "_empty"][-1]
            assert c.calc_ratio() == G[name + "_ratio"][-1]


def test_facade_mixing_raises():
    c = T.tools.Container([5, 20], 4, RT, 'diff', device=DEV)
    c.add_new_block(np.array([2, 1], np.float32))
    with pytest.raises(NotImplementedError):
        c.add_new_block_at(np.array([2, 1], np.float32), 0)
    c = T.tools.Container([5, 20], 4, RT, 'diff', device=DEV)
    c.add_new_block_at(np.array([2, 1], np.float32), 0)
    with pytest.raises(NotImplementedError):
        c.add_new_block(np.array([2, 1], np.float32))


def test_pooled_launches_do_not_grow_with_batch():
    calls = {}
    real = T.BatchedContainer._call

    def counting(self, fn, *args):
        calls['n'] = calls.get('n', 0) + 1
        return real(self, fn, *args)
    per_step = []
    try:
        T.BatchedContainer._call = counting
        for B in (3, 24):
            with lockstep_scope():
                cs = [T.tools.Container([5, 40], 6, RT, 'diff', device=DEV) for _ in range(B)]
                for i in range(6):
                    calls['n'] = 0
                    _ = [c.heightmap for c in cs]
                    x = torch.arange(B, device=DEV) % 5
                    for b, c in enumerate(cs):
                        c.add_new_block_at(np.array([1 + b % 3, 2], np.float32), x[b])
                    if i > 0:
                        per_step.append((B, calls['n']))
    finally:
        T.BatchedContainer._call = real
    counts = {n for _, n in per_step}
    assert len(counts) == 1 and counts.pop() <= 4, per_step


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("n_")])
def test_fixture_net(name):
    W, H = (int(v) for v in G[name + "_cs"])
    blocks, xs = G[name + "_blocks"], G[name + "_x"]
    n = len(xs)
    env = T.BatchedContainer(1, [W, H], n, RT, 'full', device=DEV, place_at='net')
    pnet = torch.zeros(1, 1, W, device=DEV)
    for i in range(n):
        assert np.array_equal(pnet.cpu().numpy().reshape(-1), G[name + "_pnet"][i])
        static = torch.zeros(1, 3, 1, device=DEV)
        static[0, 1:, 0] = torch.as_tensor(blocks[i].astype(np.float32))
        env.add_new_blocks_at_gather(static, torch.zeros(1, dtype=torch.int64, device=DEV),
                                     torch.as_tensor(xs[i:i + 1]), want_feature=False, pnet_out=pnet)
    assert np.array_equal(env.positions[0].cpu().numpy(), G[name + "_positions"])
    assert np.array_equal(env.stable[0].cpu().numpy().astype(np.uint8), G[name + "_stable"])
    cnt = env.counters[0].tolist()
    sc = G[name + "_scores"]
    assert (cnt[0], cnt[1], cnt[2]) == (sc[0], sc[2], sc[3]) and int(env.heightmap.max()) == sc[4]


@pytest.mark.parametrize("sem", ['container', 'net'])
def test_sweep_all_widths(sem):
    B, n = 8192, 5
    _lib.variant_hits_reset(DEV)
    for W in range(1, 65):
        for k, t in enumerate(('full', 'zero', 'diff')):
            rs = np.random.RandomState(W * 7 + k + (100 if sem == 'net' else 0))
            H = 4 * n + 2
            env = T.BatchedContainer(B, [W, H], n, RT, t, device=DEV, place_at=sem)
            m = M.PlaceAt(B, W, H, n, sem)
            form = ('full', 'zero', 'diff')[(k + W) % 3]
            pnet = torch.empty(B, 1, W, device=DEV)
            gather = bool((W + k) % 2)
            for i in range(n):
                blocks = np.stack((rs.randint(1, W + 1, B), rs.randint(1, 5, B)), 1).astype(np.int32)
                xs = rs.randint(0, W + 3, B).astype(np.int64)
                act = (rs.rand(B) < 0.8).astype(np.uint8) if i % 2 else None
                xt = torch.as_tensor(xs, device=DEV)
                at = None if act is None else torch.as_tensor(act, device=DEV)
                if gather:
                    static = torch.zeros(B, 3, 2, device=DEV)
                    static[:, 1:, 1] = torch.as_tensor(blocks.astype(np.float32), device=DEV)
                    ptr = torch.ones(B, dtype=torch.int64, device=DEV)
                    f = env.add_new_blocks_at_gather(static, ptr, xt, active=at, pnet_out=pnet, pnet_form=form)
                else:
                    f = env.add_new_blocks_at(torch.as_tensor(blocks, device=DEV), xt, active=at, pnet_out=pnet,
                                              pnet_form=form)
                m.step(blocks, xs, act)
                _compare(env, m, t, f, pnet, form)
            assert np.array_equal(env.calc_ratios64().cpu().numpy(), m.ratio())
    hits = _place_at_launches()
    sem_id = _lib.TAP_AT_NET if sem == 'net' else _lib.TAP_AT_CONTAINER
    assert {(k[2], k[4]) for k in hits if k[3] == sem_id} == {(g, a) for g in (8, 16, 32, 64) for a in (0, 1)}


def test_error_bits_and_invalid():
    B, W, H = 6, 5, 6
    env = T.BatchedContainer(B, [W, H], 4, RT, 'full', device=DEV, place_at='container')
    m = M.PlaceAt(B, W, H, 4, 'container')
    blocks = np.array([[2, 4], [6, 1], [2, 1], [0, 2], [5, 7], [1, 1]], np.int32)
    xs = np.array([0, 0, -1, 0, 3, 4], np.int64)
    for _ in range(2):
        env.add_new_blocks_at(torch.as_tensor(blocks), torch.as_tensor(xs))
        m.step(blocks, xs)
        _compare(env, m)
    assert m.err.tolist() == [1, 4, 4, 4, 1, 0]
    with pytest.raises(T.TapOverflowError):
        env.check()
    # TAP_E_INVALID: step_at on an unflagged desc, tap_env_step on a flagged one, D = 3
    L, c = _lib.lib(), _lib.ctx(DEV)
    plain = T.BatchedContainer(B, [W, H], 4, RT, 'full', device=DEV)
    x = torch.zeros(B, dtype=torch.int64, device=DEV)
    bl = torch.ones(B, 2, dtype=torch.int32, device=DEV)
    st = _lib.stream_of(torch.device(DEV))
    assert L.tap_env_step_at(c, C.byref(plain.desc), _lib.ptr(plain._state), _lib.ptr(bl), 1, None, None, _lib.ptr(x),
                             None, 0, st) == _lib.TAP_E_INVALID
    assert L.tap_env_step(c, C.byref(env.desc), _lib.ptr(env._state), _lib.ptr(bl), 1, None, None, st) == _lib.TAP_E_INVALID
    d3 = _lib.make_desc(B, [4, 4, 10], 4, RT, 'full', 'LB_GREEDY')
    d3.flags |= _lib.TAP_F_AT_CONTAINER
    blob = torch.zeros(L.tap_env_state_bytes(C.byref(d3)), dtype=torch.uint8, device=DEV)
    assert L.tap_env_step_at(c, C.byref(d3), _lib.ptr(blob), _lib.ptr(bl), 1, None, None, _lib.ptr(x), None, 0,
                             st) == _lib.TAP_E_INVALID
    big = T.BatchedContainer(2, [65, 10], 4, RT, 'full', device=DEV, place_at='net')
    with pytest.raises(T.TapError) as e:
        big.add_new_blocks_at(torch.ones(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64))
    assert e.value.status == _lib.TAP_E_UNSUPPORTED
    with pytest.raises(T.TapError):
        env.add_new_blocks(torch.ones(B, 2))
    torch.cuda.synchronize()


def _instances(B, n, seed):
    static, dynamic = synth.rand_instances(B, n, 2, seed=seed)
    tape = synth.random_feasible_tape(static, dynamic, n, seed=seed + 1)
    return static.to(DEV), dynamic.to(DEV), tape.to(DEV)


@pytest.mark.parametrize("t", ['full', 'zero', 'diff'])
def test_run_episode_tape_policies(t):
    B, n, W, H = 512, 10, 5, 60
    static, dynamic, tape = _instances(B, n, 3)
    rs = np.random.RandomState(4)
    xs = torch.as_tensor(rs.randint(0, W + 2, (B, n)), device=DEV)

    class TapeX(object):                       # replays recorded columns, one step per call
        step = 0

        def __call__(self, pin, blk):
            self.step += 1
            return xs[:, self.step - 1]
    out = T.run_episode(static, dynamic, T.TapePolicy(tape), W, H, reward_type=RT, heightmap_type=t,
                        pack_policy=TapeX(), record=True)
    st = static.cpu().numpy()
    m = M.PlaceAt(B, W, H, n, 'container')
    for i in range(n):
        p = tape[:, i].cpu().numpy()
        assert np.array_equal(out['pnet_inputs'][i].cpu().numpy().reshape(B, W).astype(np.int64), M.pnet_input(m.hm, t))
        m.step(st[np.arange(B), 1:3, p], xs[:, i].cpu().numpy())
        assert np.array_equal(out['features'][i].cpu().numpy().reshape(B, -1).astype(np.int64), M.feature(m.hm, t))
    assert np.array_equal(out['place_x'].cpu().numpy(), xs.cpu().numpy())
    assert np.array_equal(out['tour_idx'].cpu().numpy(), tape.cpu().numpy())
    assert np.array_equal(out['env'].positions.cpu().numpy(), m.positions)
    assert np.array_equal(out['reward'].cpu().numpy(), -m.ratio().astype(np.float32))
    assert 'pack_logp' not in out


def _net(W, t, seed=11):
    torch.manual_seed(seed)
    net = T.tools.DQN(W, t == 'diff')
    for bn in (net.bn1, net.bn2, net.bn3):
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
    return net.to(DEV).eval()


@pytest.mark.parametrize("t", ['full', 'diff'])
def test_run_episode_dqn_policy_and_graph(t):
    B, n, W, H = 256, 10, 5, 60
    static, dynamic, tape = _instances(B, n, 5)
    net = _net(W, t)

    def pack_policy(pin, blk):
        with torch.no_grad():
            return net(pin, blk)
    out = T.run_episode(static, dynamic, T.TapePolicy(tape), W, H, reward_type=RT, heightmap_type=t,
                        pack_policy=pack_policy)
    # host loop: the same net on the same device, the restatement as the environment
    st = static.cpu().numpy()
    m = M.PlaceAt(B, W, H, n, 'container')
    xs, lps = [], []
    for i in range(n):
        p = tape[:, i]
        blk = torch.gather(static[:, 1:, :], 2, p.view(-1, 1, 1).expand(-1, 2, 1)).transpose(2, 1)
        pin = torch.as_tensor(M.pnet_input(m.hm, t).astype(np.float32), device=DEV).unsqueeze(1)
        with torch.no_grad():
            prob = net(pin, blk)
        best = prob.max(1)
        xs.append(best[1].cpu().numpy())
        lps.append(best[0].log().cpu().numpy())
        m.step(st[np.arange(B), 1:3, p.cpu().numpy()], xs[-1])
    assert np.array_equal(out['place_x'].cpu().numpy(), np.stack(xs, 1))
    assert np.array_equal(out['pack_logp'].cpu().numpy(), np.stack(lps, 1))
    assert np.array_equal(out['env'].positions.cpu().numpy(), m.positions)
    assert np.array_equal(out['reward'].cpu().numpy(), -m.ratio().astype(np.float32))
    # the same episode captured into a hipGraph and replayed
    env = T.BatchedContainer(B, [W, H], n, RT, t, device=DEV, place_at='container')
    prev = T.pack._binary_mode
    T.pack.set_binary_check('trust')
    try:
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            T.run_episode(static, dynamic, T.TapePolicy(tape), W, H, reward_type=RT, heightmap_type=t,
                          pack_policy=pack_policy, env=env)
        torch.cuda.current_stream(DEV).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gout = T.run_episode(static, dynamic, T.TapePolicy(tape), W, H, reward_type=RT, heightmap_type=t,
                                 pack_policy=pack_policy, env=env)
        g.replay()
        torch.cuda.synchronize()
    finally:
        T.pack.set_binary_check(prev)
    assert np.array_equal(gout['place_x'].cpu().numpy(), out['place_x'].cpu().numpy())
    assert np.array_equal(gout['pack_logp'].cpu().numpy(), out['pack_logp'].cpu().numpy())
    assert np.array_equal(gout['reward'].cpu().numpy(), out['reward'].cpu().numpy())
    assert np.array_equal(env.positions.cpu().numpy(), m.positions)


def test_reward_and_render_with_pack_net(tmp_path):
    B, n, W, H = 128, 10, 5, 60
    static, dynamic, tape = _instances(B, n, 9)
    net = _net(W, 'diff', seed=12)
    st = static.cpu().numpy()
    m = M.PlaceAt(B, W, H, n, 'net')
    for i in range(n):
        p = tape[:, i].cpu().numpy()
        blk = st[np.arange(B), 1:3, p].astype(np.int64)
        pin = torch.as_tensor(M.pnet_input(m.hm, 'full').astype(np.float32), device=DEV).unsqueeze(1)
        with torch.no_grad():
            x = net(pin, torch.as_tensor(blk.astype(np.float32), device=DEV).unsqueeze(1)).max(1)[1]
        m.step(blk, x.cpu().numpy())
    ratio, scores = m.scores(n)
    for rt in ('C+P+S-SL-soft', 'C+P+S-RL-soft'):
        r = T.reward(static, tape, rt, 'bot', True, W, H, pack_net=net)
        assert np.array_equal(r.cpu().numpy(), -ratio.astype(np.float32))
    path, stem = str(tmp_path / "batch0_-1.2345.png"), str(tmp_path / "batch")    # pack.py:967 cuts 13 characters
    T.render(static, tape, path, dynamic, 0.5, pack_net=net, input_type='bot', unit=1,
             container_width=W, container_height=H, initial_container_height=H, packing_strategy='LB_GREEDY',
             reward_type=RT, allow_rot=True)
    # the ratio is fp64 arithmetic on the device (torch ops): within a few ulp of the host's, the integers exact
    np.testing.assert_allclose(np.loadtxt(stem + "-ratio.txt"), ratio, rtol=1e-14, atol=0)
    for k, name in enumerate(('valid_size', 'box_size', 'empty_size', 'stable_num', 'packing_height')):
        assert np.array_equal(np.loadtxt(stem + "-%s.txt" % name), scores[:, k].astype(np.float64))
    # without a net: unchanged (LB_GREEDY scoring, render refuses)
    r0 = T.reward(static, tape, RT, 'bot', True, W, H)
    r1 = T.reward(static, tape, 'C+P+S-lb-soft', 'bot', True, W, H)
    assert np.array_equal(r0.cpu().numpy(), r1.cpu().numpy())
    with pytest.raises(NotImplementedError):
        T.render(static, tape, path, dynamic, 0.5, input_type='bot', unit=1, container_width=W,
                 container_height=H, initial_container_height=H, packing_strategy='LB_GREEDY', reward_type=RT,
                 allow_rot=True)
    # tools.calc_positions_net on one instance of the batch
    b = 3
    blocks = st[b, 1:3, tape[b].cpu().numpy()]            # (n, 2): the advanced indices lead
    pos, _, stable, rt_, sc = T.tools.calc_positions_net(blocks, [W, H], RT, net=net, device=DEV)
    assert np.array_equal(pos, m.positions[b]) and stable == [bool(v) for v in m.stable[b]]
    assert abs(rt_ - ratio[b]) <= 1e-14 * ratio[b] and sc == scores[b].tolist()
