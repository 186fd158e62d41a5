"""The one-launch PackRNN forward on the MI355X (pack_rnn.hip: k_pack_rnn_forward<KIND>, tap_pack_rnn_forward) against the
package's float64 model (tools.PackRNN.double() on the numpy engine; tests/pack_rnn_forward_model.py has the margin rule
and its cap), its engine state against step-by-step replays of its own columns, determinism, the launch record, the
seams that take a pack-net, and the entry point's checks."""
import numpy as np
import pytest
import torch

import pack_engine_model as M
import pack_rnn_forward_model as F
import pointer_model
import tap_net_amd as T
from tap_net_amd import _lib, synth
from test_pack_rnn_forward_cpu import abi_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hits():
    h = _lib.variant_hits(DEV)
    return ({k: v for k, v in h.items() if k[0] == _lib.TAP_HIT_PACK_RNN},
            sum(v for k, v in h.items() if k[0] == _lib.TAP_HIT_PLACE_AT and k[5] == 1))


def _key(kind):
    return (_lib.TAP_HIT_PACK_RNN, 2, F.TILE, 1 if kind == 'LG' else 0, 6 if kind == 'LG' else 4, 0, 0)


def _forward(net, blocks, n):
    with torch.no_grad():
        pos, logp, neg = net(blocks.to(DEV), n)
    return pos.cpu().numpy(), logp.cpu().numpy(), -neg.cpu().numpy()


@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_against_the_float64_model(case):
    kind, W, t, n, T_, B, seed = case
    net = F.case_net(case, DEV, fused=True)
    blocks = F.make_blocks(B, T_, W, seed)
    r64 = F.run_unfolded(F.host_copy(net, torch.float64), blocks.double(), n)
    r32 = F.run_unfolded(F.host_copy(net, torch.float32), blocks, n)
    keep, whole = F.compared(r64['margin'])
    F.assert_cap(whole)
    _lib.variant_hits_reset(DEV)
    pos, logp, reward = _forward(net, blocks, n)
    assert _hits() == ({_key(kind): 1}, 0)
    assert pos.shape == (B, T_, 2) and logp.shape == (B, n) and logp.dtype == np.float32
    assert np.array_equal(pos[:, :n, 0][keep], r64['cols'][keep])
    assert np.array_equal(r32['cols'][keep], r64['cols'][keep])
    e_ref = float(np.abs(r32['logp'] - r64['logp'])[keep].max())
    err = float(np.abs(logp - r64['logp'])[keep].max())
    tol = pointer_model.tolerance(e_ref, r64['logp'][keep])
    print("logp: error %.3g, float32 torch's own %.3g, tolerance %.3g" % (err, e_ref, tol))
    assert err <= tol
    # an env the rule leaves whole: every integer and the reward are the model's
    assert np.array_equal(pos[whole], r64['pos'][whole]) and np.array_equal(reward[whole], r64['reward'][whole])
    for u in ('full', 'zero', 'diff'):
        got = np.stack([net.engines[b].get_heightap(u) for b in range(B)])
        assert np.array_equal(got[whole], r64['haps'][u][whole])
    net.reserve(B, T_, DEV).check()


def _export(eng):
    hm, pos, st, cnt = eng.env._export(True, True, True, True)
    return [x.cpu().numpy() for x in (hm, pos, st, cnt, eng.errors, eng.reward)]


@pytest.mark.parametrize("t,mb", [('full', 10), ('zero', 7), ('diff', 0)])
def test_engine_state_is_the_replay_of_its_own_columns(t, mb):
    B, n, W, Hc = 130, 15, 7, 12
    net = F.sharpen(F.seeded('G', W, seed=3, heightmap_type=t, device=DEV, fused=True, height=Hc, max_blocks_num=mb))
    blocks = F.make_blocks(B, n, W, 13, wide=0.01).to(DEV)
    with torch.no_grad():
        net(blocks, n)
    eng = net.reserve(B, n, DEV)
    cols = eng.positions[:, :n, 0].to(torch.int64)
    feat = eng.get_heightaps(t)
    dev2 = T.env.PackEngines(B, W, Hc, eng.T, t, max_blocks_num=mb, device=DEV)
    m = M.PackEngines(B, W, Hc, eng.T, t, mb)
    for i in range(n):
        f2 = dev2.step(i, blocks, cols[:, i].contiguous(), want_reward=i == n - 1)
        m.step(i, blocks.cpu().numpy(), cols[:, i].cpu().numpy(), want_reward=i == n - 1)
    for a, b in zip(_export(eng), _export(dev2)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert torch.equal(feat, f2)
    hm, pos, st, cnt, err, rw = _export(eng)
    assert np.array_equal(hm, m.hm) and np.array_equal(cnt, m.counters())
    assert np.array_equal(pos[:, :m.T], m.pos) and np.array_equal(st[:, :m.T], m.stab)
    assert np.array_equal(err, m.err) and np.array_equal(rw, m.rw64.astype(np.float32))
    assert int(np.bitwise_or.reduce(m.err)) == 1 | 4                  # overflow and a block wider than the container


def test_two_calls_and_slices_give_the_same_bytes():
    B, n, W = 130, 12, 5
    net = F.sharpen(F.seeded('LG', W, seed=3, device=DEV, fused=True))
    blocks = F.make_blocks(B, n, W, 17)
    a = _forward(net, blocks, n)
    state_a = _export(net.reserve(B, n, DEV))
    b = _forward(net, blocks, n)
    for x, y in zip(a + tuple(state_a), b + tuple(_export(net.reserve(B, n, DEV)))):
        assert np.array_equal(x, y)
    for lo, hi in ((0, 5), (64, 81)):
        part = _forward(net, blocks[lo:hi].contiguous(), n)
        for x, y in zip(a, part):
            assert x[lo:hi].tobytes() == y.tobytes()


def test_launch_record():
    B, n, W = 17, 7, 5
    blocks = F.make_blocks(B, n, W, 19)
    for kind in ('G', 'LG'):
        net = F.seeded(kind, W, seed=3, device=DEV, fused=True)
        _lib.variant_hits_reset(DEV)
        _forward(net, blocks, n)
        assert _hits() == ({_key(kind): 1}, 0)
        _forward(net, blocks[:, :, :4].contiguous(), 3)
        assert _hits() == ({_key(kind): 2}, 0)
        net.fused = False
        _lib.variant_hits_reset(DEV)
        _forward(net, blocks, n)
        assert _hits() == ({}, n)                                     # the counts of today


def _instances(B, n, seed):
    static, dynamic = synth.rand_instances(B, n, 2, seed=seed)
    tape = synth.random_feasible_tape(static, dynamic, n, seed=seed + 1)
    return static.to(DEV), dynamic.to(DEV), tape.to(DEV)


def _tour_blocks(static, tape):
    return torch.gather(static[:, 1:3, :], 2, tape.unsqueeze(1).expand(-1, 2, -1)).contiguous()


def test_run_episode_with_the_fused_net_and_graph():
    B, n, W = 256, 10, 5
    static, dynamic, tape = _instances(B, n, 41)
    net = F.sharpen(F.seeded('G', W, seed=3, device=DEV, fused=True))
    kw = dict(reward_type='C+P+S-G-soft', heightmap_type='diff', pack_rnn=net)
    # the margin rule over DRL_RNN's prefixes: an env is compared when no forward of the episode has a low-margin step
    host = F.host_copy(net, torch.float64)
    blocks = _tour_blocks(static, tape).cpu()
    whole = np.ones(B, bool)
    for k in range(1, n + 1):
        r64 = F.run_unfolded(host, blocks[:, :, :k].double().contiguous(), k)
        whole &= F.compared(r64['margin'])[1]
    F.assert_cap(whole)
    _lib.variant_hits_reset(DEV)
    with torch.no_grad():
        out = T.run_episode(static, dynamic, T.TapePolicy(tape), W, F.H, record=True, **kw)
    assert _hits() == ({_key('G'): n}, 0)
    net.fused = False
    with torch.no_grad():
        ref = T.run_episode(static, dynamic, T.TapePolicy(tape), W, F.H, record=True, **kw)
    net.fused = True
    w = torch.as_tensor(whole, device=DEV)
    assert torch.equal(out['place_x'][w], ref['place_x'][w]) and torch.equal(out['reward'][w], ref['reward'][w])
    assert np.array_equal(out['place_x'].cpu().numpy()[whole], r64['cols'][whole])
    for a, b in zip(out['features'], ref['features']):
        assert a.shape == b.shape and torch.equal(a[w], b[w])
    want = r64['logp'][whole]
    e_ref = float(np.abs(ref['pack_logp'].cpu().numpy()[whole] - want).max())
    err = float(np.abs(out['pack_logp'].cpu().numpy()[whole] - want).max())
    print("pack_logp: error %.3g, the unfused path's own %.3g" % (err, e_ref))
    assert err <= pointer_model.tolerance(e_ref, want)
    # captured into one graph and replayed: equal to eager
    prev = T.pack._binary_mode
    T.pack.set_binary_check('trust')
    try:
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s), torch.no_grad():
            T.run_episode(static, dynamic, T.TapePolicy(tape), W, F.H, **kw)
        torch.cuda.current_stream(DEV).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            gout = T.run_episode(static, dynamic, T.TapePolicy(tape), W, F.H, **kw)
        g.replay()
        torch.cuda.synchronize()
    finally:
        T.pack.set_binary_check(prev)
    for k in ('place_x', 'pack_logp', 'reward'):
        assert torch.equal(gout[k], out[k]), k
    assert any(e is gout['engine'] for e in net.captured_engines)


def test_reward_and_calc_positions_with_the_fused_net():
    B, n, W = 128, 12, 5
    static, dynamic, tape = _instances(B, n, 43)
    net = F.sharpen(F.seeded('G', W, seed=3, device=DEV, fused=True))
    r64 = F.run_unfolded(F.host_copy(net, torch.float64), torch.trunc(_tour_blocks(static, tape)).cpu().double(), n)
    whole = F.compared(r64['margin'])[1]
    F.assert_cap(whole)
    rt = 'C+P+S-G-soft'
    _lib.variant_hits_reset(DEV)
    got = T.reward(static, tape, rt, 'bot', True, W, F.H, pack_net=net)
    assert sum(_hits()[0].values()) == 1
    net.fused = False
    want = T.reward(static, tape, rt, 'bot', True, W, F.H, pack_net=net)
    assert np.array_equal(got.cpu().numpy()[whole], want.cpu().numpy()[whole])
    st = static.cpu().numpy()
    for b in np.nonzero(whole)[0][[0, 5]]:
        bl = st[b, 1:3, tape[b].cpu().numpy()]
        net.fused = True
        a = T.tools.calc_positions_net(bl, [W, F.H], rt, net=net, device=DEV)
        net.fused = False
        c = T.tools.calc_positions_net(bl, [W, F.H], rt, net=net, device=DEV)
        assert np.array_equal(a[0], c[0]) and a[2] == c[2] and a[3] == c[3] and a[4] == c[4]


def test_entry_point_checks_and_python_fallback():
    bad = [c for c in abi_cases(_lib.ctx(DEV)) if c[1] != c[2]]
    assert not bad, bad
    torch.manual_seed(5)
    net = T.tools.PackRNN(2, 64, 5, 64, 5, F.H, 'diff', pack_net_type='G', fused=True).to(DEV).eval()
    blocks = F.make_blocks(8, 6, 5, 23)
    _lib.variant_hits_reset(DEV)
    pos, logp, _ = _forward(net, blocks, 6)
    assert _hits() == ({}, 6) and logp.shape == (8, 6)               # Hb = 64 has no kernel: the torch path
    eng = T.env.PackEngines(8, 5, F.H, 6, 'full', device=DEV)
    with pytest.raises(ValueError):                                   # an engine of another form than the fold's
        T.rollout.pack_rnn_forward(F.seeded('G', 5, device=DEV).fold(), eng, blocks.to(DEV), 6)
