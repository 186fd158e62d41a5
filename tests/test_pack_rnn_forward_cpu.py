"""The one-launch PackRNN forward without a GPU (tapenv.h: tap_pack_rnn_forward): the folded algebra of the contract
(rollout.pack_rnn_forward_torch) against the unfolded torch forward (tools.PackRNN) in float64 and float32, the fall-backs
of ``fused=True``, the margin rule's cap on the GPU tests' cases, and the entry point's argument checks (they return
before any device work)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pack_engine_model as M
import pack_rnn_forward_model as F
import tap_net_amd as T
from tap_net_amd import _lib, rollout

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "pack_rnn.npz"))
FORWARDS = [str(c) for c in G["forward_cases"]]
SHARP = [('G', 5, 'diff', 10, 10), ('LG', 5, 'zero', 12, 12), ('G', 10, 'full', 7, 12), ('LG', 10, 'diff', 20, 20)]


def _parse(name):
    _, kind, w, n, t = name.split("_")
    return kind, int(w[1:]), int(n[1:]), int(t[1:])


def _folded(net, blocks, n, T_):
    eng = M.PackEngines(blocks.shape[0], net.container_width, F.H, T_, net.heightmap_type, net.max_blocks_num)
    logp, feat = rollout.pack_rnn_forward_torch(net.fold(), eng, blocks, n)
    return eng, logp.numpy(), feat


def _check_against_unfolded(net, blocks, n, T_):
    """float64: logp within 1e-10; columns, positions, reward and the three get_heightap forms equal"""
    net = F.host_copy(net, torch.float64)
    want = F.run_unfolded(net, blocks.double(), n)
    eng, logp, feat = _folded(net, blocks.double(), n, T_)
    assert logp.dtype == np.float64 and np.abs(logp - want['logp']).max() <= 1e-10
    assert np.array_equal(eng.pos[:, :n, 0], want['cols'])
    assert np.array_equal(eng.pos[:, :n], want['pos'][:, :n]) and not want['pos'][:, n:].any()
    assert np.array_equal(eng.reward.numpy(), want['reward'])
    for t in ('full', 'zero', 'diff'):
        assert np.array_equal(M.heightap(eng.hm, t), want['haps'][t])
    assert np.array_equal(feat.numpy()[:, :, 0], want['haps'][net.heightmap_type])


@pytest.mark.parametrize("name", FORWARDS)
def test_folded_float64_matches_unfolded_on_the_fixture(name):
    kind, W, bn, Tn = _parse(name)
    _check_against_unfolded(F.seeded(kind, W), torch.from_numpy(G[name + "_blocks"]), bn, Tn)


@pytest.mark.parametrize("case", SHARP, ids=lambda c: "%s-w%d-%s-n%d-t%d" % c)
def test_folded_float64_matches_unfolded_sharpened(case):
    kind, W, t, n, T_ = case
    net = F.sharpen(F.seeded(kind, W, seed=3, heightmap_type=t))
    _check_against_unfolded(net, F.make_blocks(64, T_, W, 11), n, T_)


@pytest.mark.parametrize("name", FORWARDS)
def test_folded_float32_matches_the_fixture(name):
    kind, W, bn, Tn = _parse(name)
    eng, logp, _ = _folded(F.seeded(kind, W), torch.from_numpy(G[name + "_blocks"]), bn, Tn)
    assert logp.dtype == np.float32
    np.testing.assert_allclose(logp, G[name + "_logp"], rtol=0, atol=1e-5)
    if G[name + "_margin"] > 1e-4:
        assert np.array_equal(eng.pos[:, :Tn], G[name + "_positions"])


def test_fold_shapes_and_cache():
    for kind, D in (('G', 256), ('LG', 384)):
        net = F.seeded(kind, 5)
        f = net.fold()
        assert (f.kind, f.Hb, f.Hh, f.D, f.W, f.Wp, f.heightmap_type) == (kind, 128, 128, D, 5, 4, 'diff')
        assert tuple(f.Pe.shape) == (384, 2) and tuple(f.Pd_e.shape) == (3 * D, 128) and tuple(f.Pd_h.shape) == (3 * D, 4)
        assert (f.Pd_b is None) == (kind == 'G') and all(getattr(f, k) is None or getattr(f, k).is_contiguous() for k in _lib.PACK_RNN_WEIGHTS)
        assert net.fold() is f
        f.weights('cpu')                                             # the launch's struct: addresses, not copied with the net
        twin = copy.deepcopy(net)
        assert twin._fold is None and twin.fold() is not f and torch.equal(twin.fold().Pe, f.Pe)
        with torch.no_grad():
            net.fc[2].bias.add_(1)
        assert net.fold() is not f                                   # a parameter changed: folded again
        assert list(net.state_dict()) == [str(k) for k in G["sd_%s_keys" % kind]]
        assert net.double().fold().Pe.dtype == torch.float64


def test_fused_falls_back_to_the_torch_path():
    """off the GPU, in train(), or with outputs that need a gradient, fused=True is the torch path: its bytes"""
    blocks = F.make_blocks(8, 6, 5, 5)
    plain = F.seeded('G', 5, seed=4)
    fused = F.seeded('G', 5, seed=4, fused=True)
    assert fused.fused and not plain.fused
    assert not fused._takes_launch(blocks, fused.reserve(8, 6, 'cpu'))        # host blocks
    with torch.no_grad():
        a, b = plain(blocks, 6), fused(blocks, 6)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, b = plain(blocks, 6), fused(blocks, 6)                                # grad enabled: hit_porb_log needs one
    assert b[1].requires_grad and all(torch.equal(x, y) for x, y in zip(a, b))
    plain.train(), fused.train()
    torch.manual_seed(0)
    a = plain(blocks, 6)
    torch.manual_seed(0)
    b = fused(blocks, 6)                                                     # the same dropout draws
    assert all(torch.equal(x, y) for x, y in zip(a, b))

    class FakeGpu(object):                                                   # what _takes_launch reads of the blocks
        is_cuda, dtype, requires_grad = True, torch.float32, False
    with torch.no_grad():
        assert not fused._takes_launch(FakeGpu(), fused.reserve(8, 6, 'cpu'))    # train()
        fused.eval()
        assert not fused._takes_launch(FakeGpu(), fused.reserve(8, 6, 'cpu'))    # not an env.PackEngines
        FakeGpu.dtype = torch.float64
        assert not fused._takes_launch(FakeGpu(), None)
    assert T.tools.load_pack_net.__defaults__[-1] is False


def test_double_net_on_a_host_engine_is_the_float64_model():
    net = F.seeded('LG', 5, seed=4).double()
    with torch.no_grad():
        pos, logp, neg = net(F.make_blocks(4, 5, 5, 2).double(), 5)
    assert logp.dtype == torch.float64 and pos.dtype == torch.int32 and neg.dtype == torch.float32


@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_margin_cap_holds_on_the_gpu_cases(case):
    """the cap is a condition on the float64 model alone; torch's own float32 path stays inside it too: it differs from
    the float64 model in no compared step"""
    kind, W, t, n, T_, B, seed = case
    net = F.case_net(case)
    blocks = F.make_blocks(B, T_, W, seed)
    r64 = F.run_unfolded(F.host_copy(net, torch.float64), blocks.double(), n)
    r32 = F.run_unfolded(net, blocks, n)
    keep, whole = F.compared(r64['margin'])
    F.assert_cap(whole)
    assert np.array_equal(r32['cols'][keep], r64['cols'][keep])
    assert np.array_equal(r32['pos'][whole], r64['pos'][whole]) and np.array_equal(r32['reward'][whole], r64['reward'][whole])


def test_margin_cap_of_the_issue():
    """sharpened nets, seed 3, B = 512, n = 10, W 5 and 10, G and LG: at most 2 % of the envs have a low-margin step, and
    torch's float32 forward differs from the float64 one in none of the others"""
    for kind in ('G', 'LG'):
        for W in (5, 10):
            net = F.sharpen(F.seeded(kind, W, seed=3))
            blocks = F.make_blocks(512, 10, W, 7)
            r64 = F.run_unfolded(F.host_copy(net, torch.float64), blocks.double(), 10)
            r32 = F.run_unfolded(net, blocks, 10)
            keep, whole = F.compared(r64['margin'])
            F.assert_cap(whole)
            assert np.array_equal(r32['cols'][whole], r64['cols'][whole])


# ---- C ABI ------------------------------------------------------------------------------------------------------------

def abi_cases(ctx=None):
    """every TAP_E_INVALID / TAP_E_UNSUPPORTED case of tap_pack_rnn_forward, with made-up addresses: each returns before
    any device work.  -> [(what, got, wanted)]"""
    L = _lib.lib()
    E, U = _lib.TAP_E_INVALID, _lib.TAP_E_UNSUPPORTED
    out = []

    def weights(kind=_lib.TAP_PACK_G, Hb=128, Hh=128, W=5, form=_lib.TAP_FEAT_DIFF, **ptrs):
        w = _lib.PackRnnWeights()
        w.kind, w.Hb, w.Hh, w.W, w.form = kind, Hb, Hh, W, form
        for k in _lib.PACK_RNN_WEIGHTS:
            setattr(w, k, ptrs.get(k, None if k == 'Pd_b' and kind == _lib.TAP_PACK_G else 4096))
        return w

    def desc(B=4, W=5, n_max=10, place='net'):
        d = _lib.make_desc(B, [W, 50], n_max, 'C+P+S-G-soft', 'diff', 'LB_GREEDY')
        return _lib.set_place_at(d, place) if place else d

    def call(what, wanted, d=None, w=None, state=4096, blocks=4096, T_=5, n=5, mb=10, logp=4096, reward=4096, feat=None, nod=False, now=False):
        d = desc() if d is None else d
        w = weights() if w is None else w
        got = L.tap_pack_rnn_forward(ctx, None if nod else C.byref(d), C.c_void_p(state), C.c_void_p(blocks), T_, n, mb,
                                     None if now else C.byref(w), C.c_void_p(logp), C.c_void_p(reward), C.c_void_p(feat), None)
        out.append((what, got, wanted))
    call("null descriptor", E, nod=True)
    call("null weights", E, now=True)
    call("unflagged descriptor", E, d=desc(place=None))
    call("TAP_AT_CONTAINER descriptor", E, d=desc(place='container'))
    call("blocks_num 0", E, n=0)
    call("blocks_num above T", E, n=6)
    call("T 0", E, T_=0, n=0)
    call("max_blocks -1", E, mb=-1)
    call("B 0", _lib.TAP_OK, d=desc(B=0), state=0, blocks=0, logp=0, reward=0)
    call("null state", E, state=0)
    call("null blocks", E, blocks=0)
    call("null logp_out", E, logp=0)
    call("null reward_out", E, reward=0)
    call("null fc2_w", E, w=weights(fc2_w=None))
    call("LG without Pd_b", E, w=weights(kind=_lib.TAP_PACK_LG, Pd_b=None))
    call("weights of another W", E, w=weights(W=6))
    call("misaligned state", E, state=4096 + 8)
    call("misaligned blocks", E, blocks=4096 + 2)
    call("misaligned feature_out", E, feat=4096 + 1)
    call("misaligned Pd_h", E, w=weights(Pd_h=4096 + 2))
    call("Hb 64", U, w=weights(Hb=64))
    call("Hh 64", U, w=weights(Hh=64))
    call("kind 2", U, w=weights(kind=2))
    call("form 3", U, w=weights(form=3))
    call("T beyond the tape", U, T_=11, n=5)
    call("W 1", U, d=desc(W=1), w=weights(W=1))
    return out


def test_entry_point_rejects_without_device_work():
    assert "tap_pack_rnn_forward" in _lib.EXPORTS
    bad = [c for c in abi_cases() if c[1] != c[2]]
    assert not bad, bad
