"""The global pack-net's engine on the MI355X (place_at.hip: k_place_at<G, true, true>, tap_env_step_engine): every
integer output bit-exact and the reward equal to the numpy restatement's (tests/pack_engine_model.py, which
tests/test_pack_rnn_cpu.py pins to the reference's traces); tools.PackRNN, reward / render / calc_positions_net and
run_episode(pack_rnn=...) against the same network on the restatement."""
import os

import numpy as np
import pytest
import torch

import pack_engine_model as M
import tap_net_amd as T
from tap_net_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "pack_rnn.npz"))
FORWARDS = [str(c) for c in G["forward_cases"]]
H = 60


def _engine_launches():
    return sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == _lib.TAP_HIT_PLACE_AT and k[5] == 1)


def _compare(eng, m, t, feat, reward=True):
    hm, pos, st, cnt = eng.env._export(True, True, True, True)
    assert np.array_equal(hm.cpu().numpy(), m.hm)
    assert np.array_equal(cnt.cpu().numpy(), m.counters())
    assert np.array_equal(pos.cpu().numpy()[:, :m.T], m.pos)
    assert np.array_equal(st.cpu().numpy()[:, :m.T], m.stab)
    assert np.array_equal(eng.errors.cpu().numpy(), m.err)
    if feat is not None:
        assert np.array_equal(feat.cpu().numpy()[:, :, 0].astype(np.int64), M.heightap(m.hm, t))
    if reward:
        assert np.array_equal(eng.reward.cpu().numpy(), m.rw64.astype(np.float32))


def test_sweep_all_widths_with_wraps():
    B, n = 8192, 25
    _lib.variant_hits_reset(DEV)
    launches, seen = 0, 0
    for W in range(2, 65):
        for k, t in enumerate(('full', 'zero', 'diff')):
            rs = np.random.RandomState(W * 3 + k)
            Hc = 30 + (W % 3) * 15                                 # some containers overflow (error bit 1)
            mb = (10, 10, 0, 7)[(W + k) % 4]
            eng = T.env.PackEngines(B, W, Hc, n, t, max_blocks_num=mb, device=DEV)
            m = M.PackEngines(B, W, Hc, n, t, mb)
            blocks = np.stack((rs.randint(1, W + 1, (B, n)) + (rs.rand(B, n) < 0.2) * 0.5,
                               rs.randint(1, 5, (B, n)) + (rs.rand(B, n) < 0.2) * 0.75), 1).astype(np.float32)
            widths = blocks[:, 0, :]
            widths[rs.rand(B, n) < 0.01] = W + 1                         # wider than the container: error bit 4
            bt = torch.as_tensor(blocks, device=DEV)
            for i in range(n):
                xs = rs.randint(-1 if i % 5 == 4 else 0, W + 3, B).astype(np.int64)
                want = i % 3 != 1
                f = eng.step(i, bt, torch.as_tensor(xs, device=DEV), want_reward=want)
                launches += 1
                m.step(i, blocks, xs, want_reward=want)
                _compare(eng, m, t, f, reward=want)
                seen |= int(np.bitwise_or.reduce(m.err))
    assert seen == 1 | 4                                           # both divergences exercised
    assert _engine_launches() == launches
    keys = {k for k in _lib.variant_hits(DEV) if k[0] == _lib.TAP_HIT_PLACE_AT}
    assert {k[2] for k in keys} == {8, 16, 32, 64} and {(k[3], k[4], k[5]) for k in keys} == {(_lib.TAP_AT_NET, 0, 1)}


@pytest.mark.parametrize("W", (2, 5, 7, 10, 16, 31, 64))
def test_fixture_traces(W):
    name = "e_w%d" % W
    blocks, xs = G[name + "_blocks"], G[name + "_x"]
    n = len(xs)
    bt = torch.as_tensor(blocks.T[None].copy(), device=DEV)
    for t in ('full', 'zero', 'diff'):
        eng = T.env.PackEngines(1, W, H, n, t, device=DEV)
        for i in range(n):
            f = eng.step(i, bt, torch.as_tensor(xs[i:i + 1], device=DEV))
            assert eng.reward[0].item() == np.float32(G[name + "_rw"][i])
            assert np.array_equal(f.cpu().numpy()[0, :, 0], G[name + "_hap_" + t][i]), (t, i)
            for u in ('full', 'zero', 'diff'):
                assert np.array_equal(eng.get_heightaps(u).cpu().numpy()[0, :, 0], G[name + "_hap_" + u][i])
        assert np.array_equal(eng.positions[0].cpu().numpy(), G[name + "_pos"])
        assert np.array_equal(eng.stable[0].cpu().numpy().astype(np.uint8), G[name + "_stable"])
        eng.check()


def _seeded(kind, W, seed=None, engine=None, device=DEV):
    torch.manual_seed(1000 + 10 * W + (1 if kind == 'LG' else 0) if seed is None else seed)
    net = T.tools.PackRNN(2, 128, W, 128, W, H, 'diff', pack_net_type=kind, engine=engine)
    return net.to(device).eval()


@pytest.mark.parametrize("name", FORWARDS)
def test_pack_rnn_device_vs_host(name):
    _, kind, w, bn, tn = name.split("_")
    W, bn = int(w[1:]), int(bn[1:])
    blocks = torch.from_numpy(G[name + "_blocks"])
    host = _seeded(kind, W, engine=M.factory(), device='cpu')
    dev = _seeded(kind, W)
    with torch.no_grad():
        hp, hl, hr = host(blocks, bn)
        dp, dl, dr = dev(blocks.to(DEV), bn)
    # log-probs up to the first step whose column differs (none may differ where the top-2 margin exceeds 1e-4)
    same = (dp.cpu().numpy()[:, :bn, 0] == hp.numpy()[:, :bn, 0]).all(axis=0)
    k = bn if same.all() else int(np.argmin(same)) + 1
    np.testing.assert_allclose(dl.cpu().numpy()[:, :k], hl.numpy()[:, :k], rtol=0, atol=1e-5)
    if G[name + "_margin"] > 1e-4:
        assert k == bn
        assert np.array_equal(dp.cpu().numpy(), hp.numpy())
        assert np.array_equal(dr.cpu().numpy(), hr.numpy())
        for t in ('full', 'zero', 'diff'):
            got = np.stack([dev.engines[b].get_heightap(t) for b in range(6)])
            assert np.array_equal(got, np.stack([host.engines[b].get_heightap(t) for b in range(6)]))


def _instances(B, n, seed):
    static, dynamic = synth.rand_instances(B, n, 2, seed=seed)
    tape = synth.random_feasible_tape(static, dynamic, n, seed=seed + 1)
    return static.to(DEV), dynamic.to(DEV), tape.to(DEV)


def _host_scores(net, static, tape, W):
    """calc_positions_LG_net for every sample on the restatement: the net's forward (same device, numpy engine), then
    the replay without a wrap"""
    B, n = tape.shape
    st = static.cpu().numpy()
    blocks = np.stack([st[b, 1:3, tape[b].cpu().numpy()].T for b in range(B)]).astype(int).astype(np.float32)
    net.engine_factory, net._engine = M.factory(), None
    try:
        with torch.no_grad():
            pos, _, _ = net(torch.as_tensor(blocks, device=DEV), n)
    finally:
        net.engine_factory, net._engine = T.env.PackEngines, None
    rep = M.PackEngines(B, W, H, n, 'full', 0)
    for t in range(n):
        rep.step(t, blocks, pos[:, t, 0], want_reward=False, want_input=False)
    mh = rep.hm.max(axis=1)
    ratio = (rep.valid / (mh * W).astype(np.float64) + rep.valid / (rep.valid + rep.empty).astype(np.float64)
             + rep.nstable / np.float64(n)) / 3
    scores = np.stack((rep.valid, mh * W, rep.empty, rep.nstable, mh), 1)
    return rep, ratio, scores


@pytest.mark.parametrize("kind", ['G', 'LG'])
def test_reward_render_calc_positions_with_pack_rnn(kind, tmp_path):
    B, n, W = 128, 12, 5
    rt = 'C+P+S-%s-soft' % kind
    static, dynamic, tape = _instances(B, n, 21 if kind == 'G' else 22)
    net = _seeded(kind, W, seed=5)
    rep, ratio, scores = _host_scores(net, static, tape, W)
    r = T.reward(static, tape, rt, 'bot', True, W, H, pack_net=net)
    assert np.array_equal(r.cpu().numpy(), -ratio.astype(np.float32))
    path, stem = str(tmp_path / "batch0_-1.2345.png"), str(tmp_path / "batch")
    T.render(static, tape, path, dynamic, 0.5, pack_net=net, input_type='bot', unit=1, container_width=W,
             container_height=H, initial_container_height=H, packing_strategy='LB_GREEDY', reward_type=rt,
             allow_rot=True)
    np.testing.assert_allclose(np.loadtxt(stem + "-ratio.txt"), ratio, rtol=1e-14, atol=0)
    for k, fname in enumerate(('valid_size', 'box_size', 'empty_size', 'stable_num', 'packing_height')):
        assert np.array_equal(np.loadtxt(stem + "-%s.txt" % fname), scores[:, k].astype(np.float64))
    # without a net: unchanged (LB_GREEDY scoring, render refuses)
    r0 = T.reward(static, tape, rt, 'bot', True, W, H)
    assert np.array_equal(r0.cpu().numpy(), T.reward(static, tape, 'C+P+S-lb-soft', 'bot', True, W, H).cpu().numpy())
    with pytest.raises(NotImplementedError):
        T.render(static, tape, path, dynamic, 0.5, input_type='bot', unit=1, container_width=W, container_height=H,
                 initial_container_height=H, packing_strategy='LB_GREEDY', reward_type=rt, allow_rot=True)
    # tools.calc_positions_net on one instance, routed to calc_positions_LG_net (its -gt- twin too); the restatement
    # runs the same batch of one, so both forwards are the same device ops
    st = static.cpu().numpy()
    for b, r_ in ((3, rt), (7, 'C+P+S-%s-gt-soft' % kind)):
        rep1, ratio1, scores1 = _host_scores(net, static[b:b + 1], tape[b:b + 1], W)
        blocks = st[b, 1:3, tape[b].cpu().numpy()]
        pos, _, stable, ratio_b, sc = T.tools.calc_positions_net(blocks, [W, H], r_, net=net, device=DEV)
        assert np.array_equal(pos, rep1.pos[0]) and stable == [bool(v) for v in rep1.stab[0]]
        assert abs(ratio_b - ratio1[0]) <= 1e-14 * ratio1[0] and sc == scores1[0].tolist()


def test_calc_positions_net_reproduces_the_fixture():
    """the package's calc_positions_net (-> calc_positions_LG_net, the G and -gt- routes) against the reference's
    calc_positions_LG_net on the fixture's seeded cases whose top-2 margin leaves no argmax to float rounding"""
    checked = 0
    for name in [str(c) for c in G["calc_cases"] if str(c).startswith("c_seeded")]:
        if G[name + "_margin"] <= 1e-4:
            continue
        kind = name.split("_")[2]
        net = _seeded(kind, 5)
        for rt in ('C+P+S-%s-soft' % kind, 'C+P+S-%s-gt-soft' % kind):
            pos, _, st, ratio, sc = T.tools.calc_positions_net(G[name + "_blocks"], [5, H], rt, net=net, device=DEV)
            assert np.array_equal(pos, G[name + "_positions"]) and st == [bool(v) for v in G[name + "_stable"]], name
            assert abs(ratio - G[name + "_ratio"]) <= 1e-14 * G[name + "_ratio"], name
            assert sc == G[name + "_scores"].tolist(), name
        checked += 1
    assert checked >= 4


def test_engine_out_buffer_is_checked():
    eng = T.env.PackEngines(8, 5, H, 4, 'diff', device=DEV)
    blocks = torch.ones(8, 2, 4, device=DEV)
    x = torch.zeros(8, dtype=torch.int64, device=DEV)
    for bad in (torch.empty(8, 5, 1, device=DEV), torch.empty(8, 4, 1, dtype=torch.float64, device=DEV),
                torch.empty(8, 4, 2, device=DEV)[:, :, :1], torch.empty(8, 4, 1)):
        with pytest.raises(ValueError):
            eng.step(0, blocks, x, out=bad)
    out = torch.empty(8, 4, 1, device=DEV)
    assert eng.step(0, blocks, x, out=out) is out
    torch.cuda.synchronize()


@pytest.mark.parametrize("t", ['diff', 'full'])
def test_run_episode_pack_rnn_and_graph(t):
    B, n, W = 256, 10, 5
    static, dynamic, tape = _instances(B, n, 31)
    torch.manual_seed(9)
    net = T.tools.PackRNN(2, 128, W, 128, W, H, t, pack_net_type='G').to(DEV).eval()
    counts = []
    real = T.env.PackEngines.step

    def counting(self, *a, **k):
        counts[-1] += 1
        return real(self, *a, **k)

    def policy(step, **kw):
        counts.append(0)
        return tape[:, step]
    _lib.variant_hits_reset(DEV)
    T.env.PackEngines.step = counting
    try:
        with torch.no_grad():
            out = T.run_episode(static, dynamic, policy, W, H, reward_type='C+P+S-G-soft', heightmap_type=t,
                                pack_rnn=net, record=True)
    finally:
        T.env.PackEngines.step = real
    assert counts == list(range(1, n + 1))                     # t engine launches at the t-th outer step
    assert _engine_launches() == n * (n + 1) // 2
    # the same loop on the host engine, the same network on the device
    host = T.tools.PackRNN(2, 128, W, 128, W, H, t, pack_net_type='G', engine=M.factory()).to(DEV).eval()
    host.load_state_dict(net.state_dict())
    from tap_net_amd import rollout
    masks = T.MaskStepper(static, dynamic, 'bot', True, False)
    with torch.no_grad():
        ref = rollout.rnn_loop(lambda step, **kw: tape[:, step], masks, host, t, n, record=True)
    assert torch.equal(out['tour_idx'], tape)
    assert torch.equal(out['place_x'].cpu(), ref['place_x'].cpu())
    assert np.array_equal(out['reward'].cpu().numpy(), ref['reward'].cpu().numpy())
    np.testing.assert_allclose(out['pack_logp'].cpu().numpy(), ref['pack_logp'].cpu().numpy(), rtol=0, atol=1e-5)
    for a, b in zip(out['features'], ref['features']):
        assert torch.equal(a.cpu(), b.cpu())
    # captured into a hipGraph and replayed: equal to eager
    prev = T.pack._binary_mode
    T.pack.set_binary_check('trust')
    try:
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s), torch.no_grad():
            T.run_episode(static, dynamic, T.TapePolicy(tape), W, H, reward_type='C+P+S-G-soft', heightmap_type=t,
                          pack_rnn=net)
        torch.cuda.current_stream(DEV).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            gout = T.run_episode(static, dynamic, T.TapePolicy(tape), W, H, reward_type='C+P+S-G-soft',
                                 heightmap_type=t, pack_rnn=net)
        g.replay()
        torch.cuda.synchronize()
    finally:
        T.pack.set_binary_check(prev)
    assert torch.equal(gout['place_x'], out['place_x'])
    assert torch.equal(gout['pack_logp'], out['pack_logp'])
    assert torch.equal(gout['reward'], out['reward'])
    # the captured engine stays alive with the net after another batch size replaced the net's current engine
    captured = gout.pop('engine')
    assert any(e is captured for e in net.captured_engines)
    del captured
    T.reward(static[:64], tape[:64], 'C+P+S-G-soft', 'bot', True, W, H, pack_net=net)
    assert net.reserve(64, n, DEV).batch_size == 64
    gout['place_x'].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gout['place_x'], out['place_x'])
    assert torch.equal(gout['reward'], out['reward'])
