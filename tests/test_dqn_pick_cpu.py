"""The one-launch L-Pnet pick without a GPU: DQN.fold and rollout.dqn_pick_torch in float64 against the unfolded net, the
fold's cache, the reference's state-dict keys, pick's fallback, the loader's ``fused``, the C-ABI row and the reference's
recorded outputs (tests/golden/dqn_pick.npz, make_golden_dqn_pick.py)."""
import copy
import os
import pickle
import re

import numpy as np
import pytest
import torch

import dqn_pick_model as DM
import tap_net_amd as T
from tap_net_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "dqn_pick.npz"))

# tools.DQN's state dict in the reference (tools.py:3322-3338): 27 keys
REF_KEYS = ['conv_height_map.weight', 'conv_height_map.bias', 'conv_block.weight', 'conv_block.bias',
            'bn1.weight', 'bn1.bias', 'bn1.running_mean', 'bn1.running_var', 'bn1.num_batches_tracked',
            'conv2.weight', 'conv2.bias', 'bn2.weight', 'bn2.bias', 'bn2.running_mean', 'bn2.running_var', 'bn2.num_batches_tracked',
            'conv3.weight', 'conv3.bias', 'bn3.weight', 'bn3.bias', 'bn3.running_mean', 'bn3.running_var', 'bn3.num_batches_tracked',
            'lin1.weight', 'lin1.bias', 'head.weight', 'head.bias']


@pytest.mark.parametrize("case", DM.CASES + [(3, False), (13, True)], ids=DM.case_id)
def test_fold_reproduces_the_net_in_float64(case):
    W, diff = case
    net = DM.seeded(W, diff, dtype=torch.float64)
    hm, blk = DM.inputs(W, diff, 7)
    with torch.no_grad():
        want = net(hm.double(), blk.double())
    f = net.fold()
    assert (f.W, f.Wm, f.P) == (W, W - 1 if diff else W, (W - 1 if diff else W) + 2)
    assert f.L1.shape == (512, 256 * f.P) and f.W2.dtype == torch.float64
    x, logp, probs = T.rollout.dqn_pick_torch(f, hm.double(), blk.double(), want_probs=True)
    best = want.max(1)
    assert float((probs - want).abs().max()) <= 1e-12
    assert torch.equal(x, best[1])
    assert float((logp - best[0].log()).abs().max()) <= 1e-12
    if W > 2:
        wide = DM.inputs(W, diff, 64)
        assert len(set(T.rollout.dqn_pick_torch(f, wide[0].double(), wide[1].double())[0].tolist())) >= 2


def test_l1_is_position_major_and_operands_are_packed():
    net = DM.seeded(5, True)
    f = net.fold()
    w = net.lin1.weight.detach()
    for o, c, p in ((0, 0, 1), (17, 200, 5), (511, 255, 0)):
        assert f.L1[o, p * 256 + c] == w[o, c * f.P + p]
    for X, Xp, T_, KS in ((f.W2, f.W2p, 32, 2), (f.W3, f.W3p, 32, 2), (f.L1, f.L1p, 16, 4)):
        N, K = X.shape
        assert Xp.shape == (K // (4 * KS), N // T_, 64, 4) and Xp.is_contiguous()
        for q, t, l, i in ((0, 0, 0, 0), (1, 2, 37, 3), (K // (4 * KS) - 1, N // T_ - 1, 63, 2)):
            assert Xp[q, t, l, i] == X[t * T_ + l % T_, KS * (4 * q + i) + l // T_]


def test_fold_cache_follows_parameters_and_running_stats():
    net = DM.seeded(5, True)
    f = net.fold()
    assert net.fold() is f
    with torch.no_grad():
        net.conv2.weight.mul_(1.5)
    g = net.fold()
    assert g is not f and not torch.equal(g.W2, f.W2)
    with torch.no_grad():
        net.bn3.running_var.add_(0.25)
    h = net.fold()
    assert h is not g and not torch.equal(h.W3, g.W3)
    net.bn2.eps = 1e-3
    assert net.fold() is not h
    clone = pickle.loads(pickle.dumps(net))
    assert clone._fold is None and clone.fused is net.fused
    k = clone.fold()
    assert k is not net.fold() and torch.equal(k.L1, net.fold().L1)
    assert copy.deepcopy(net)._fold is None
    with pytest.raises(RuntimeError):
        net.train().fold()


@pytest.mark.parametrize("diff", [True, False])
def test_reference_keys_load_strictly(diff):
    src = DM.seeded(5, diff)
    assert list(src.state_dict()) == REF_KEYS
    net = T.tools.DQN(5, diff, fused=True)
    net.load_state_dict({k: v.clone() for k, v in src.state_dict().items()}, strict=True)
    assert net.fused is True and len(list(net.buffers())) == 9 and len(list(net.parameters())) == 18
    assert list(net.state_dict()) == REF_KEYS


@pytest.mark.parametrize("fused", [False, True])
def test_pick_on_the_host_is_the_forward(fused):
    net = DM.seeded(5, True, fused=fused)
    hm, blk = DM.inputs(5, True, 9)
    with torch.no_grad():
        x, logp = net.pick(hm, blk)
        best = net(hm, blk).max(1)
    assert x.dtype == torch.int64 and torch.equal(x, best[1])
    assert torch.equal(logp, best[0].log())


def test_fused_is_the_default_and_adds_no_state():
    net = T.tools.DQN(5, True)
    assert net.fused is True and T.tools.DQN(5, True, fused=False).fused is False
    assert list(net.state_dict()) == REF_KEYS


def test_loader_sets_fused(monkeypatch):
    sd = DM.seeded(5, True).state_dict()
    monkeypatch.setattr(os.path, "exists", lambda p: True)
    monkeypatch.setattr(torch, "load", lambda *a, **k: sd)
    for rt in ('C+P+S-SL-soft', 'C+P+S-RL-soft'):
        net = T.tools.load_pack_net(rt, 5, device=None, fused=True)
        assert isinstance(net, T.tools.DQN) and net.fused is True and not net.training and net.is_diff_height
        assert T.tools.load_pack_net(rt, 5, device=None).fused is False
    assert "ignore" not in T.tools.load_pack_net.__doc__


def test_c_abi_row():
    L = _lib.lib()
    header = open(_lib.HEADER_PATH).read()
    for name in ("tap_dqn_pick", "tap_dqn_pick_geometry"):
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert len(_lib._PROTOS["tap_dqn_pick"][1]) == 11
    assert _lib.TAP_HIT_DQN == 33
    assert _lib.DqnWeights._fields_[:4] == [(k, _lib.C.c_int32) for k in ("W", "Wm", "P", "reserved")]


def test_geometry_and_support():
    assert _lib.dqn_pick_geometry(5, True)[:2] == (16, 6)
    assert _lib.dqn_pick_geometry(5, False)[:2] == (16, 7)
    assert _lib.dqn_pick_geometry(9, True)[:2] == (8, 10)
    assert all(_lib.dqn_pick_geometry(W, d)[2] <= 160 * 1024 for W in range(2, 13) for d in (True, False))
    assert all(T.rollout.dqn_pick_supported(W, d) for W in range(2, 11) for d in (True, False))
    assert not T.rollout.dqn_pick_supported(64, True) and not T.rollout.dqn_pick_supported(1, False)


def test_null_weights_are_refused_without_a_device():
    L = _lib.lib()
    assert L.tap_dqn_pick(None, None, None, 0, None, 0, 4, None, None, None, None) == _lib.TAP_E_INVALID
    w = _lib.DqnWeights()
    w.W, w.Wm, w.P = 5, 4, 7                                               # P disagrees
    assert L.tap_dqn_pick(None, _lib.C.byref(w), None, 0, None, 0, 4, None, None, None, None) == _lib.TAP_E_INVALID
    w.P = 6
    assert L.tap_dqn_pick(None, _lib.C.byref(w), None, 0, None, 0, 0, None, None, None, None) == _lib.TAP_OK
    assert L.tap_dqn_pick(None, _lib.C.byref(w), None, 0, None, 0, 4, None, None, None, None) == _lib.TAP_E_INVALID


@pytest.mark.parametrize("key", [str(c) for c in G["cases"]])
def test_fold_matches_the_reference_outputs(key):
    W, diff = next(c for c in DM.CASES if DM.case_id(c) == key)
    net = DM.seeded(W, diff)
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in G[key + "_sd_keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in G[key + "_sd_shapes"]]
    hm, blk = DM.inputs(W, diff, 64)
    assert np.array_equal(hm.numpy(), G[key + "_hm"]) and np.array_equal(blk.numpy(), G[key + "_block"])
    f = copy.deepcopy(net).double().fold()
    x, logp, probs = T.rollout.dqn_pick_torch(f, hm.double(), blk.double(), want_probs=True)
    got = float(np.abs(probs.numpy() - G[key + "_out"].astype(np.float64)).max())
    err = float(G[key + "_err"])
    assert 0 < err < 1e-5
    assert got <= err + 1e-12, (got, err)
    keep = DM.compared(probs)
    assert np.array_equal(x.numpy()[keep], G[key + "_out"].argmax(1)[keep])
