"""The pack-net placement without a GPU: the numpy restatement (tests/place_at_model.py) against the reference's traces
(tests/golden/place_at.npz, make_golden_place_at.py), tools.DQN against the reference's network, the C ABI's new
symbols and the state-blob sizes of place-at descriptors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import place_at_model as M
import ref_loader
import tap_net_amd as T
from tap_net_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "place_at.npz"))
CASES = [str(c) for c in G["cases"]]


def _container_trace(name):
    W, H = (int(v) for v in G[name + "_cs"])
    blocks, xs = G[name + "_blocks"], G[name + "_x"]
    t = name.rsplit("_", 1)[1]
    m = M.PlaceAt(1, W, H, len(xs), 'container')
    for i in range(len(xs)):
        m.step(blocks[i:i + 1], xs[i:i + 1])
        assert np.array_equal(M.feature(m.hm, t)[0], G[name + "_feature"][i]), (name, i)
        assert np.array_equal(m.hm[0], G[name + "_hm"][i]), (name, i)
        assert m.valid[0] == G[name + "_valid"][i] and m.empty[0] == G[name + "_empty"][i], (name, i)
        assert m.ratio()[0] == G[name + "_ratio"][i], (name, i)
    assert np.array_equal(m.positions[0], G[name + "_positions"])
    assert np.array_equal(m.stable[0], G[name + "_stable"])
    assert m.err[0] == 0


def _net_trace(name):
    W, H = (int(v) for v in G[name + "_cs"])
    blocks, xs = G[name + "_blocks"], G[name + "_x"]
    m = M.PlaceAt(1, W, H, len(xs), 'net')
    for i in range(len(xs)):
        assert np.array_equal(M.pnet_input(m.hm, 'full')[0].astype(np.float32), G[name + "_pnet"][i]), (name, i)
        assert np.array_equal(blocks[i].astype(np.float32), G[name + "_netblock"][i])
        m.step(blocks[i:i + 1], xs[i:i + 1])
    ratio, scores = m.scores(len(xs))
    assert np.array_equal(m.positions[0], G[name + "_positions"])
    assert np.array_equal(m.stable[0], G[name + "_stable"])
    assert np.array_equal(scores[0], G[name + "_scores"])
    assert ratio[0] == G[name + "_ratio"]


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("c_")])
def test_restatement_container_fixture(name):
    _container_trace(name)


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("n_")])
def test_restatement_net_fixture(name):
    _net_trace(name)


def test_fixture_covers_the_issue():
    widths = {int(G[c + "_cs"][0]) for c in CASES}
    assert widths == {1, 2, 5, 7, 10, 16, 31, 64}
    assert {c.rsplit("_", 1)[1] for c in CASES if c.startswith("c_")} == {"full", "zero", "diff"}
    clamps = sum(int((G[c + "_x"] + G[c + "_blocks"][:, 0] > G[c + "_cs"][0]).sum()) for c in CASES)
    assert clamps > 20
    assert any(G[c + "_stable"].min() == 0 for c in CASES if c.startswith("n_"))     # the NET seam's stability test bites


def test_pnet_forms():
    hm = np.array([[3, 1, 4, 1, 5]])
    assert M.pnet_input(hm, 'diff').tolist() == [[-2, 3, -3, 4, 0]]
    assert M.pnet_input(hm, 'zero').tolist() == [[2, 0, 3, 0, 4]]
    assert M.feature(hm, 'diff').tolist() == [[-2, 3, -3, 4]]


def _seeded(diff):
    torch.manual_seed(7 if diff else 8)
    net = T.tools.DQN(5, diff)
    for bn in (net.bn1, net.bn2, net.bn3):
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
    return net.eval()


@pytest.mark.parametrize("diff", [True, False])
def test_dqn_matches_reference_outputs(diff):
    key = "dqn_%s" % ("diff" if diff else "full")
    net = _seeded(diff)
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in G[key + "_sd_keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in G[key + "_sd_shapes"]]
    with torch.no_grad():
        y = net(torch.from_numpy(G[key + "_hm"]), torch.from_numpy(G[key + "_block"]))
    np.testing.assert_allclose(y.numpy(), G[key + "_out"], rtol=0, atol=1e-6)


def test_dqn_generalises_width():
    net = T.tools.DQN(9, True).eval()
    with torch.no_grad():
        y = net(torch.zeros(3, 1, 9), torch.ones(3, 1, 2))
    assert tuple(y.shape) == (3, 9)
    assert net.lin1.in_features == 256 * 10
    assert T.tools.DQN(5, False).lin1.in_features == 1792


@pytest.mark.reference
@pytest.mark.skipif(not ref_loader.available(), reason="reference checkout not present")
@pytest.mark.parametrize("diff", [True, False])
def test_dqn_loads_reference_state_dict(diff):
    tools = ref_loader.load()[0]
    torch.manual_seed(3)
    ref = tools.DQN(5, diff).eval()
    for bn in (ref.bn1, ref.bn2, ref.bn3):
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2.0)
    ours = T.tools.DQN(5, diff)
    ours.load_state_dict(ref.state_dict(), strict=True)
    ours.eval()
    hm, blk = torch.randn(16, 1, 5) * 3, torch.randint(1, 5, (16, 1, 2)).float()
    with torch.no_grad():
        np.testing.assert_allclose(ours(hm, blk).numpy(), ref(hm, blk).numpy(), rtol=0, atol=1e-6)


@pytest.mark.reference
@pytest.mark.skipif(not ref_loader.available(), reason="reference checkout not present")
@pytest.mark.parametrize("seed", range(6))
def test_restatement_live_vs_reference(seed):
    tools = ref_loader.load()[0]
    rs = np.random.RandomState(100 + seed)
    W = int(rs.choice([1, 3, 5, 8, 13, 33, 64]))
    t = ['full', 'zero', 'diff'][seed % 3]
    n, H = 15, 100
    blocks = np.stack((rs.randint(1, W + 1, size=n), rs.randint(1, 6, size=n)), 1)
    xs = rs.randint(0, W + 5, size=n)
    c = tools.Container([W, H], n, 'C+P+S-RL-soft', t)
    m = M.PlaceAt(1, W, H, n, 'container')
    for i in range(n):
        f = np.asarray(c.add_new_block_at(blocks[i].astype(np.float32), int(xs[i])), np.int64).reshape(-1)
        m.step(blocks[i:i + 1], xs[i:i + 1])
        assert np.array_equal(M.feature(m.hm, t)[0], f)
        assert (m.valid[0], m.empty[0]) == (c.valid_size, c.empty_size)
        assert m.ratio()[0] == c.calc_ratio()
    assert np.array_equal(m.positions[0], c.positions)
    assert m.stable[0].tolist() == [int(v) for v in c.stable]
    # the NET seam on a live calc_one_position_net, step by step
    blocks_i = blocks.astype(int)
    pos, st = np.zeros((n, 2), int), [False] * n
    hm, cont = np.zeros(W, int), np.zeros((W, H))
    valid = empty = 0
    mn = M.PlaceAt(1, W, H, n, 'net')

    class Net(object):
        def __init__(self, x):
            self.x = x

        def __call__(self, *_):
            p = torch.zeros(1, W + 5)
            p[0, self.x] = 1
            return p
    real = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for i in range(n):
            pos, cont, st, hm, valid, empty, _ = tools.calc_one_position_net(
                blocks_i, i, pos, cont, 'C+P+S-SL-soft', st, hm, valid, empty, None, Net(int(xs[i])))
            mn.step(blocks[i:i + 1], xs[i:i + 1])
            assert np.array_equal(mn.hm[0], hm) and mn.valid[0] == valid and mn.empty[0] == empty
    finally:
        torch.Tensor.cuda = real
    assert np.array_equal(mn.positions[0], pos)
    assert mn.stable[0].tolist() == [int(v) for v in st]


# ---- C ABI --------------------------------------------------------------------------------------------------------

def test_new_symbols_exported():
    L = _lib.lib()
    for name in ("tap_env_desc_set_place_at", "tap_env_step_at", "tap_env_step_at_gather"):
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None
    assert L.tap_abi_version() == 1


def _bytes(d):
    return _lib.lib().tap_env_state_bytes(C.byref(d))


@pytest.mark.parametrize("B,W,n", [(1, 5, 10), (7, 1, 3), (8192, 5, 10), (300, 64, 40), (33, 17, 20)])
def test_state_bytes(B, W, n):
    d = _lib.make_desc(B, [W, 50], n, 'C+P+S-SL-soft', 'diff', 'LB_GREEDY')
    base = _bytes(d)
    assert d.flags & (_lib.TAP_F_AT_CONTAINER | _lib.TAP_F_AT_NET) == 0          # never from the reward string
    for sem in ('container', 'net'):
        f = _lib.make_desc(B, [W, 50], n, 'C+P+S-SL-soft', 'diff', 'LB_GREEDY')
        _lib.set_place_at(f, sem)
        assert _bytes(f) == base + ((B * W * 4 + 255) // 256) * 256
        _lib.set_place_at(f, None)
        assert _bytes(f) == base


def test_set_place_at_rules():
    d = _lib.make_desc(4, [5, 5, 50], 10, 'C+P+S-SL-soft', 'full', 'LB_GREEDY')
    assert _lib.lib().tap_env_desc_set_place_at(C.byref(d), _lib.TAP_AT_NET) == _lib.TAP_E_INVALID    # 3D
    d = _lib.make_desc(4, [5, 50], 10, 'C+P+S-SL-soft', 'full', 'LB_GREEDY')
    assert _lib.lib().tap_env_desc_set_place_at(C.byref(d), 3) == _lib.TAP_E_INVALID
    assert _lib.lib().tap_env_desc_set_place_at(C.byref(d), _lib.TAP_AT_NET) == _lib.TAP_OK
    assert d.flags & _lib.TAP_F_AT_NET
    assert _lib.lib().tap_env_desc_set_place_at(C.byref(d), _lib.TAP_AT_CONTAINER) == _lib.TAP_OK
    assert d.flags & (_lib.TAP_F_AT_CONTAINER | _lib.TAP_F_AT_NET) == _lib.TAP_F_AT_CONTAINER
    with pytest.raises(ValueError):
        _lib.set_place_at(d, 'voxel')


def test_step_at_rejects_without_device_work():
    """argument checks that return before any device work (null ctx: no HIP device needed)"""
    L = _lib.lib()
    d = _lib.make_desc(4, [5, 50], 10, 'C+P+S-SL-soft', 'full', 'LB_GREEDY')
    assert L.tap_env_step_at(None, C.byref(d), None, None, 0, None, None, None, None, 0, None) == _lib.TAP_E_INVALID
    assert L.tap_env_step_at_gather(None, C.byref(d), None, None, 3, 10, None, None, None, None, None, 0, None) == _lib.TAP_E_INVALID
    _lib.set_place_at(d, 'net')
    assert L.tap_env_step(None, C.byref(d), None, None, 0, None, None, None) == _lib.TAP_E_INVALID
    assert L.tap_env_step_gather(None, C.byref(d), None, None, 3, 10, None, None, None, None) == _lib.TAP_E_INVALID
    d.D, d.L = 3, 1
    assert L.tap_env_step_at(None, C.byref(d), None, None, 0, None, None, None, None, 0, None) == _lib.TAP_E_INVALID
