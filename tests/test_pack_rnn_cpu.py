"""The global pack-net (G / LG PackRNN, the reference's DRL_RNN) without a GPU: the numpy engine
(tests/pack_engine_model.py) against the reference's traces (tests/golden/pack_rnn.npz, make_golden_pack_rnn.py),
tools.PackRNN on that engine against the reference's forwards, calc_positions_LG_net's replay and DRL_RNN's loop,
and the C ABI's new entry point."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pack_engine_model as M
import ref_loader
import tap_net_amd as T
from tap_net_amd import _lib, rollout

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "pack_rnn.npz"))
ENGINE_WIDTHS = (2, 5, 7, 10, 16, 31, 64)
FORWARDS = [str(c) for c in G["forward_cases"]]
CALCS = [str(c) for c in G["calc_cases"]]
H = 60


def seeded(kind, W, seed=None, engine=None):
    """tools.PackRNN with the weights the fixture's seeded reference net got (same layers, same construction order)"""
    torch.manual_seed(1000 + 10 * W + (1 if kind == 'LG' else 0) if seed is None else seed)
    net = T.tools.PackRNN(2, 128, W, 128, W, H, 'diff', pack_net_type=kind,
                          engine=M.factory() if engine is None else engine)
    return net.eval()


def parse(name):
    _, kind, w, n, t = name.split("_")
    return kind, int(w[1:]), int(n[1:]), int(t[1:])


# ---- the engine restatement -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", ENGINE_WIDTHS)
def test_restatement_engine_fixture(W):
    name = "e_w%d" % W
    blocks, xs = G[name + "_blocks"], G[name + "_x"]
    n = len(xs)
    for t in ('full', 'zero', 'diff'):
        e = M.PackEngines(1, W, H, n, t, 10, grid=True)            # grid: LG_RL's add_block / is_stable_2d literally
        bl = blocks.T[None].astype(np.float32)                      # (1, 2, n)
        for i in range(n):
            out = e.step(i, bl, xs[i:i + 1])
            assert e.rw64[0] == G[name + "_rw"][i], (W, i)
            assert e.reward[0].item() == np.float32(G[name + "_rw"][i])
            assert np.array_equal(e.pre_hm[0], G[name + "_hm"][i]), (W, i)
            assert (e.pre_valid[0], e.pre_empty[0]) == (G[name + "_valid"][i], G[name + "_empty"][i]), (W, i)
            assert np.array_equal(out.numpy()[0, :, 0], G[name + "_hap_" + t][i]), (W, t, i)
            for u in ('full', 'zero', 'diff'):
                assert np.array_equal(e.get_heightaps(u).numpy()[0, :, 0], G[name + "_hap_" + u][i])
        assert np.array_equal(e.pos[0], G[name + "_pos"])
        assert np.array_equal(e.stab[0], G[name + "_stable"])
        assert e.err[0] == 0


def test_engine_fixture_covers_the_issue():
    assert {int(G["e_w%d_cs" % W][0]) for W in ENGINE_WIDTHS} == set(ENGINE_WIDTHS)
    clamps = sum(int((G["e_w%d_x" % W] + np.trunc(G["e_w%d_blocks" % W][:, 0]) > W).sum()) for W in ENGINE_WIDTHS)
    assert clamps > 20
    assert sum(int((G["e_w%d_stable" % W] == 0).sum()) for W in ENGINE_WIDTHS) > 10       # the stability test bites
    for W in ENGINE_WIDTHS:                                                               # the wraps after 10 and 20
        assert not G["e_w%d_hap_full" % W][[9, 19]].any() and G["e_w%d_hap_full" % W][[8, 18]].any()
        # empty = sum(hm) - valid, the TAP_AT_NET rule, on every reference step
        assert np.array_equal(G["e_w%d_empty" % W], G["e_w%d_hm" % W].sum(1) - G["e_w%d_valid" % W])


def test_is_stable_2d_literal():
    assert M.is_stable_2d([5], 3, 1) and not M.is_stable_2d([-1], 3, 1) and not M.is_stable_2d([0], 3, 1)
    assert M.is_stable_2d([0, 4, 4, 0], 0, 4) and not M.is_stable_2d([4, 0, 0, 0], 0, 4)
    assert not M.is_stable_2d([-1, 0, 2], 1, 3)


# ---- tools.PackRNN on the numpy engine ------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ['G', 'LG'])
def test_state_dict_names_and_shapes(kind):
    sd = seeded(kind, 5, seed=0).state_dict()
    assert list(sd) == [str(k) for k in G["sd_%s_keys" % kind]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in G["sd_%s_shapes" % kind]]


@pytest.mark.parametrize("name", FORWARDS)
def test_forward_matches_reference(name):
    kind, W, bn, Tn = parse(name)
    net = seeded(kind, W)
    with torch.no_grad():
        pos, logp, neg = net(torch.from_numpy(G[name + "_blocks"]), bn)
    assert tuple(pos.shape) == (6, Tn, 2)
    assert np.array_equal(pos.numpy().astype(np.int64), G[name + "_positions"])
    np.testing.assert_allclose(logp.numpy(), G[name + "_logp"], rtol=0, atol=1e-6)
    assert np.array_equal(neg.numpy(), G[name + "_neg_reward"])
    for t in ('full', 'zero', 'diff'):
        got = np.stack([net.engines[b].get_heightap(t) for b in range(len(net.engines))])
        assert got.dtype == np.float64 and np.array_equal(got, G[name + "_hap_" + t])
    with pytest.raises(IndexError):
        net.engines[6]


def test_forward_reuses_its_engine():
    net = seeded('G', 5)
    built = []
    f = M.factory()
    net.engine_factory = lambda *a: built.append(a) or f(*a)
    blocks = torch.from_numpy(G["f_G_w5_n12_t12_blocks"])
    with torch.no_grad():
        for t in range(1, 13):                      # DRL_RNN's growing prefixes
            net(blocks[:, :, :t].contiguous(), t)
        a = net(blocks, 12)
        b = net(blocks, 12)
    assert len(built) <= 5
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def _calc_np(net, blocks, W):
    """LG_RL.calc_positions on the numpy engine: the forward, then the replay without a wrap"""
    n = len(blocks)
    bl = torch.from_numpy(blocks.astype(int).astype(np.float32).T[None].copy())
    with torch.no_grad():
        pos, _, neg = net(bl, n)
    rep = M.PackEngines(1, W, H, n, 'full', 0, grid=True)
    for t in range(n):
        rep.step(t, bl, pos[:, t, 0], want_reward=False, want_input=False)
    mh = int(rep.hm[0].max())
    valid, empty, nst = int(rep.valid[0]), int(rep.empty[0]), int(rep.nstable[0])
    ratio = (valid / np.float64(mh * W) + valid / np.float64(valid + empty) + nst / np.float64(n)) / 3
    return rep.pos[0], rep.stab[0], ratio, [valid, mh * W, empty, nst, mh], neg.numpy()[0]


def _check_calc(name, net):
    pos, st, ratio, scores, neg = _calc_np(net, G[name + "_blocks"], 5)
    assert np.array_equal(pos, G[name + "_positions"]) and np.array_equal(st, G[name + "_stable"])
    assert ratio == G[name + "_ratio"] and scores == G[name + "_scores"].tolist()
    assert neg == G[name + "_neg_reward"]


@pytest.mark.parametrize("name", [c for c in CALCS if c.startswith("c_seeded")])
def test_calc_positions_seeded(name):
    _check_calc(name, seeded(name.split("_")[2], 5))


def test_calc_fixture_pins_the_wrap():
    for src in ('seeded_LG', 'ckpt_G'):
        name = "c_%s_n15" % src
        assert np.float32(-G[name + "_ratio"]) != G[name + "_neg_reward"]    # the engine wrapped, the replay did not
    for name in CALCS:
        if not name.endswith("n15"):
            assert np.float32(-G[name + "_ratio"]) == G[name + "_neg_reward"]


def _reference_checkpoint():
    return os.path.join(ref_loader.REFERENCE_DIR, "pretrain_model", "G_rand_diff", "actor.pt")


@pytest.mark.reference
@pytest.mark.skipif(not ref_loader.available(), reason="reference checkout not present")
def test_g_checkpoint_loads_strictly_and_reproduces(tmp_path, monkeypatch):
    d = tmp_path / "pack_net" / "G_rand_diff" / "checkpoints" / "199"
    d.mkdir(parents=True)
    os.symlink(_reference_checkpoint(), str(d / "actor.pt"))
    monkeypatch.chdir(tmp_path)
    net = T.tools.load_pack_net('C+P+S-G-soft', 5, device=None)           # strict load_state_dict
    assert isinstance(net, T.tools.PackRNN) and net.pack_net_type == 'G' and not net.training
    net.engine_factory = M.factory()
    for name in [c for c in CALCS if c.startswith("c_ckpt")]:
        _check_calc(name, net)
    with pytest.raises(FileNotFoundError):
        T.tools.load_pack_net('C+P+S-LG-soft', 5, device=None)


def test_lg_checkpoint_is_missing(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for rt in ('C+P+S-LG-soft', 'C+P+S-LG-gt-soft', 'C+P+S-G-soft', 'C+P+S-G-gt-soft'):
        with pytest.raises(FileNotFoundError):
            T.tools.load_pack_net(rt, 5)
    assert T.tools.PACK_NET_CHECKPOINTS['C+P+S-G-gt-soft'] == './pack_net/G_rand_diff/checkpoints/199/actor.pt'
    assert T.tools.PACK_NET_CHECKPOINTS['C+P+S-LG-soft'] == './pack_net/LG_rand_diff/checkpoints/199/actor.pt'


# ---- DRL_RNN's loop --------------------------------------------------------------------------------------------------

class _NoPrecedence(object):
    """the MaskStepper surface for instances without precedence (the fixture's dynamic is all zeros)"""

    def __init__(self, static):
        self.static = static
        self.dynamic = self.current_mask = self.mask = None

    def step(self, ptr):
        pass


def test_rnn_loop_matches_drl_rnn():
    static = torch.from_numpy(G["drl_static"])
    tour = torch.from_numpy(G["drl_tour_idx"])
    n = tour.shape[1]
    net = seeded('G', 5, seed=2024)

    def policy(step, **kw):
        return tour[:, step]
    with torch.no_grad():
        out = rollout.rnn_loop(policy, _NoPrecedence(static), net, 'diff', n, record=True, check=False)
    assert torch.equal(out['tour_idx'], tour)
    np.testing.assert_allclose(out['pack_logp'].numpy(), G["drl_pack_logp"], rtol=0, atol=1e-6)
    assert np.array_equal(out['reward'].numpy(), G["drl_scores"])
    assert len(out['features']) == n
    for t in range(n):
        assert np.array_equal(out['features'][t].numpy()[:, :, 0], G["drl_decoder_dynamic"][t]), t
    assert out['engine'].launches == n * (n + 1) // 2
    assert tuple(out['place_x'].shape) == (4, n)


# ---- C ABI ------------------------------------------------------------------------------------------------------------

def test_new_symbol_exported():
    L = _lib.lib()
    assert "tap_env_step_engine" in _lib.EXPORTS and getattr(L, "tap_env_step_engine") is not None
    assert L.tap_abi_version() == 1
    with pytest.raises(Exception):
        _lib.make_desc(4, [5, 50], 10, 'C+P+S-G-soft', 'diff', 'PNET')


def test_step_engine_rejects_without_device_work():
    """argument checks that return before any device work (null ctx: no HIP device needed)"""
    L = _lib.lib()
    E = _lib.TAP_E_INVALID

    def call(d, T_=5, step=0, mb=10, blocks=1):
        return L.tap_env_step_engine(None, C.byref(d), None, C.c_void_p(blocks) if blocks else None, T_, step, mb,
                                     None, None, None, None)
    d = _lib.make_desc(4, [5, 50], 10, 'C+P+S-G-soft', 'diff', 'LB_GREEDY')
    assert call(d) == E                                         # unflagged
    _lib.set_place_at(d, 'container')
    assert call(d) == E                                         # TAP_AT_CONTAINER
    _lib.set_place_at(d, 'net')
    assert call(d, step=5) == E and call(d, step=-1) == E       # outside [0, T)
    assert call(d, T_=12, step=10) == E                         # beyond the tape (n_max = 10)
    assert call(d, mb=-1) == E and call(d, T_=0) == E
    assert call(d, blocks=0) == E                               # null blocks
    assert L.tap_env_step_engine(None, None, None, None, 5, 0, 10, None, None, None, None) == E
    d.D, d.L = 3, 1
    assert call(d) == E


def test_python_argument_checks():
    with pytest.raises(ValueError):
        T.env.PackEngines(4, 5, 50, 10, 'voxel')
    with pytest.raises(ValueError):
        T.env.PackEngines(4, 5, 50, 10, 'diff', max_blocks_num=-1)
    with pytest.raises(NotImplementedError):
        T.tools.calc_positions_LG_net(np.ones((3, 2)), [5, 50], 'C+P+S-SL-soft')
    with pytest.raises(NotImplementedError):
        T.tools.load_pack_net('C+P+S-lb-soft', 5)
    net = seeded('G', 5)
    static = torch.zeros(2, 3, 4)
    with pytest.raises(TypeError):
        T.pack._episode_scores_pack_net(static, torch.zeros(2, 4, dtype=torch.int64), 'C+P+S-G-soft', [5, 50],
                                        T.tools.DQN(5, True), 'bot', True)
    with pytest.raises(ValueError):
        T.run_episode(static, torch.zeros(2, 6, 4), None, 7, 50, pack_rnn=net)
    with pytest.raises(ValueError):                     # the net's width is not the container's
        T.pack.episode_scores_rnn(static, torch.zeros(2, 4, dtype=torch.int64), [7, 50], net)


def test_engine_tape_growth_stops_at_the_descriptor_limit():
    net = seeded('G', 5)
    assert net.reserve(2, 3000, 'cpu').T == 3000
    assert net.reserve(2, 3001, 'cpu').T == 4096                  # doubling capped at n_max's limit
    assert net.reserve(2, 10, 'cpu').T == 4096                    # a shorter sequence reuses it
    assert net.reserve(3, 10, 'cpu').T == 10                      # another batch size: sized afresh
    assert net.captured_engines == []
