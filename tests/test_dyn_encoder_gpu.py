"""The dynamic encoder on the bit shadow on the MI355X (encode.hip: k_encode_bits<HPL>, k_encode_bits_bw_partial,
k_encode_bits_bw_reduce) against the numpy model of tests/dyn_encoder_model.py.

The forward is compared with ``np.array_equal``: the contract fixes the order of the fp32 additions, so the device
gives the model's bytes (up to the sign of a zero, which ``==`` does not see).  Against ``F.conv1d`` in float64 and for
the backward the bounds are the derived ones: n sequential or reordered fp32 additions err by at most
n * 2^-24 * sum |terms| (tests/test_dyn_encoder_cpu.py: test_model_against_float64 has the derivation)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dyn_encoder_model as M
import oracle_lib as O
import tap_net_amd as T
from tap_net_amd import _lib, pack, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (rows, nR, H, B): every value of each axis at least once (test_case_list_covers_every_axis); one and two shadow planes;
# one and two hidden rows per lane (HPL 2: one plane and H > 64) with one and several hidden chunks (128 hidden rows per
# chunk at HPL 2, 64 at HPL 1) and a last chunk that is not full; windows wider than a pass (32 columns at HPL 2, 64 at
# HPL 1): nR 68 and 256; and -- (10, 4, 7, 2050) -- more than one env per workgroup with a ragged last one (the launcher
# gives a workgroup B // 1024 consecutive envs)
CASES = [(10, 4, 1, 1), (30, 20, 128, 67), (63, 60, 7, 3), (64, 68, 64, 3), (65, 20, 130, 3), (126, 60, 128, 1),
         (128, 256, 130, 3), (30, 256, 130, 3), (10, 4, 7, 2050), (30, 20, 300, 3)]
DENSITIES = (0.0, 0.05, 0.5, 1.0)


def _keys(extra):
    return {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_ENCODE_BITS and k[5] == extra}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _encode(bits, W, b, rows=None):
    with torch.no_grad():
        return T.encode_dynamic_bits(_dev(bits), _dev(W), _dev(b), rows=rows).cpu().numpy()


def _hpl(rows, H):
    return 2 if rows <= 64 and H > 64 else 1


def test_case_list_covers_every_axis():
    assert {c[0] for c in CASES} == {10, 30, 63, 64, 65, 126, 128}
    assert {c[1] for c in CASES} == {4, 20, 60, 68, 256}
    assert {c[2] for c in CASES} == {1, 7, 64, 128, 130, 300}
    assert {c[3] for c in CASES} == {1, 3, 67, 2050}
    # every instantiation the launcher can pick: (hidden rows per lane, planes) -- two planes always run one row per lane
    assert {(_hpl(c[0], c[2]), M.planes_of(c[0])) for c in CASES} == {(1, 1), (2, 1), (1, 2)}


@pytest.mark.parametrize("rows,nR,H,B", CASES)
def test_forward_is_the_models_bytes(rows, nR, H, B):
    _lib.variant_hits_reset(DEV)
    for i, density in enumerate(DENSITIES):
        for bias in (True, False):
            dyn, bits, W, b = M.random_case(B, rows, nR, H, density, 100 * rows + nR + i, bias=bias)
            want = M.encode(bits, W, b, rows, nR)
            got = _encode(bits, W, b)
            assert got.dtype == np.float32 and got.shape == (B, H, nR)
            assert np.array_equal(got, want), (density, bias, np.argwhere(got != want)[:4])
            if density == 0.0:                                     # an all-zero shadow gives exactly the bias
                assert np.array_equal(got, np.broadcast_to((b if bias else np.zeros(H, np.float32))[None, :, None], got.shape))
            # garbage at the positions >= rows changes nothing; the (B, planes, nR) view and the Conv1d weight
            # (H, rows, 1) are the same call
            junk = M.garbage(bits, rows, nR, 7)
            assert np.array_equal(_encode(junk, W, b), want)
            g3 = _encode(bits.reshape(B, M.planes_of(rows), nR), W[:, :, None], b)
            assert np.array_equal(g3, want)
    planes = M.planes_of(rows)
    assert _keys(0) == {(_lib.TAP_HIT_ENCODE_BITS, 0, _hpl(rows, H), planes, bb, 0, 0) for bb in (0, 1)}, _keys(0)


@pytest.mark.parametrize("rows,nR,H,B", CASES[:8])
def test_forward_agrees_with_conv1d_in_float64(rows, nR, H, B):
    """the reference's own arithmetic (an nn.Conv1d with kernel_size 1) in float64 on the CPU, on the expanded tensor"""
    dyn, bits, W, b = M.random_case(B, rows, nR, H, 0.3, 9 * rows + H)
    got = _encode(bits, W, b).astype(np.float64)
    want = F.conv1d(torch.from_numpy(dyn.astype(np.float64)), torch.from_numpy(W.astype(np.float64))[:, :, None],
                    torch.from_numpy(b.astype(np.float64))).numpy()
    bound = rows * M.U32 * (np.abs(W.astype(np.float64)).sum(1) + np.abs(b.astype(np.float64)))
    assert (np.abs(got - want) <= bound[None, :, None]).all()
    tame = np.arange(H) != H // 2                                  # every row but the spiky one: the bound is a tight one there
    assert (bound[tame] <= 2e-3).all() and (H == 1 or tame.any())    # 128 * 2^-24 * (sum of 128 |randn| + |b|) ~ 8e-4


# (B, rows, nR, H): the issue's three (one env per slice each), then the path a training batch takes -- several envs
# per slice, accumulators carried from env to env, a ragged last slice: B = 2050 in one hidden chunk (3 envs per slice,
# 684 slices, the last one holds one env), and B = 700 in three hidden chunks of 31 rows (1024 // 3 = 341 slices wanted: 3 envs per
# slice, 234 slices, the last one holds one env)
BW_CASES = [(1, 30, 20, 7), (67, 65, 68, 130), (3, 128, 256, 64), (2050, 10, 4, 7), (700, 128, 4, 64)]


def _bw_inputs(B, rows, nR, H, seed):
    dyn, bits, W, b = M.random_case(B, rows, nR, H, 0.4, seed, spiky=False)
    g = np.random.RandomState(seed + 1).randn(B, H, nR).astype(np.float32)
    return bits, W, b, g


def _bw_raw(bits, g, B, rows, nR, H, want_bias=True):
    L, c = _lib.lib(), _lib.ctx(torch.device(DEV))
    need = L.tap_encode_bits_backward_scratch(B, nR, rows, H)
    scratch = torch.full((need // 4 + 4,), float('nan'), device=DEV)
    dW = torch.full((H, rows), float('nan'), device=DEV)
    db = torch.full((H,), float('nan'), device=DEV) if want_bias else None
    _lib.check(L.tap_encode_bits_backward(c, _lib.ptr(bits), _lib.ptr(g), B, nR, rows, H, _lib.ptr(dW), _lib.ptr(db),
                                          _lib.ptr(scratch), need, _lib.stream_of(torch.device(DEV))), c)
    return dW.cpu().numpy(), None if db is None else db.cpu().numpy()


@pytest.mark.parametrize("B,rows,nR,H", BW_CASES)
def test_backward(B, rows, nR, H):
    bits, W, b, g = _bw_inputs(B, rows, nR, H, 50 + rows)
    dW64, db64, dWm, dbm = M.backward64(bits, g, rows, nR)
    K = B * nR                                                     # terms per element; the bound holds for ANY summation order
    tb, tg = _dev(bits), _dev(g)
    _lib.variant_hits_reset(DEV)
    dW, db = _bw_raw(tb, tg, B, rows, nR, H)
    assert np.isfinite(dW).all() and np.isfinite(db).all()
    assert (np.abs(dW - dW64) <= K * M.U32 * dWm).all(), np.abs(dW - dW64).max()
    assert (np.abs(db - db64) <= K * M.U32 * dbm).all(), np.abs(db - db64).max()
    dW2, db2 = _bw_raw(tb, tg, B, rows, nR, H)                     # deterministic: the same bytes
    assert dW.tobytes() == dW2.tobytes() and db.tobytes() == db2.tobytes()
    dW3, none = _bw_raw(tb, tg, B, rows, nR, H, want_bias=False)   # dbias NULL
    assert none is None and dW3.tobytes() == dW.tobytes()
    P = M.planes_of(rows)
    assert _keys(1) == {(_lib.TAP_HIT_ENCODE_BITS, 0, 0, P, 1, 1, 0), (_lib.TAP_HIT_ENCODE_BITS, 0, 0, P, 0, 1, 0)}
    # through autograd: the same values; the caller's bits overwritten between forward and backward change nothing
    tw, tbias = _dev(W).requires_grad_(True), _dev(b).requires_grad_(True)
    mine = tb.clone()
    out = T.encode_dynamic_bits(mine, tw, tbias)
    assert out.requires_grad and np.array_equal(out.detach().cpu().numpy(), M.encode(bits, W, b, rows, nR))
    mine.fill_(-1)
    out.backward(tg)
    assert tw.grad.cpu().numpy().tobytes() == dW.tobytes() and tbias.grad.cpu().numpy().tobytes() == db.tobytes()
    # a bias that needs no gradient, a Conv1d-shaped weight (H, rows, 1): the gradient takes the weight's shape
    w3 = _dev(W[:, :, None]).requires_grad_(True)
    T.encode_dynamic_bits(tb, w3, _dev(b)).backward(tg)
    assert tuple(w3.grad.shape) == (H, rows, 1) and w3.grad.cpu().numpy().tobytes() == dW.tobytes()


def test_empty_batch_and_offset_views():
    """B == 0 through the wrapper (the C entries answer TAP_OK without a launch): an empty output, zero gradients; and a
    shadow that is an 8-byte aligned view into a larger buffer"""
    W, b = torch.randn(7, 30, device=DEV, requires_grad=True), torch.randn(7, device=DEV, requires_grad=True)
    empty = torch.zeros(0, 20, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        assert tuple(T.encode_dynamic_bits(empty, W, b).shape) == (0, 7, 20)
    out = T.encode_dynamic_bits(empty, W, b)
    out.sum().backward()
    assert tuple(out.shape) == (0, 7, 20) and not W.grad.any() and not b.grad.any()
    dyn, bits, Wn, bn = M.random_case(3, 30, 20, 7, 0.3, 5)
    flat = torch.zeros(3 * 20 + 1, dtype=torch.int64, device=DEV)
    view = flat[1:].view(3, 20)                                    # 8 bytes past a 16-byte boundary
    view.copy_(_dev(bits))
    assert view.data_ptr() % 16 == 8
    with torch.no_grad():
        got = T.encode_dynamic_bits(view, _dev(Wn), _dev(bn)).cpu().numpy()
    assert np.array_equal(got, M.encode(bits, Wn, bn, 30, 20))
    # a second backward through the custom launch fails loudly instead of returning nothing
    w2 = _dev(Wn).requires_grad_(True)
    o2 = T.encode_dynamic_bits(_dev(bits), w2)
    g1, = torch.autograd.grad(o2.sum(), w2, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


# ---- on the step object ---------------------------------------------------------------------------------------------
class _Scorer(object):
    """logits = v . tanh(encoder(shadow)); ``bits_of()`` is where the shadow comes from"""

    def __init__(self, enc, v, bits_of, keep=True):
        self.enc, self.v, self.bits_of, self.keep = enc, v, bits_of, keep
        self.hidden = []

    def __call__(self, step, **_):
        if step == 0:
            self.hidden = []
        hid = self.enc(self.bits_of())
        if self.keep:
            self.hidden.append(hid.clone())
        return (torch.tanh(hid) * self.v[None, :, None]).sum(1)


def _window(D):
    """c2's window (2D, n = 10: rows 30, nR 20) or a 3D window with two planes (n = 22: rows 66, nR 132), B = 64"""
    n = 10 if D == 2 else 22
    static, dynamic = synth.rand_instances(64, n, D, seed=60 + D)
    cs = [5, 50] if D == 2 else [5, 5, 200]
    return n, static.to(DEV).contiguous(), dynamic.to(DEV).contiguous(), cs


def _encoder(rows, H, seed):
    torch.manual_seed(seed)
    enc = T.DynamicBitsEncoder(rows, H).to(DEV)
    v = torch.randn(H, device=DEV)
    return enc, v


def _episode(D, lean, enc, v, keep=True):
    n, static, dynamic, cs = _window(D)
    env = T.BatchedContainer(64, cs, n, "C+P+S-lb-soft", "diff", device=DEV)
    sp = T.EpisodeStepper(static, dynamic, env, 'bot', True, steps=n, expand_dynamic=not lean)
    bits_of = (lambda: sp.dynamic_bits) if lean else (lambda: pack.dynamic_bits(sp.dynamic)[0])
    scorer = _Scorer(enc, v, bits_of, keep)
    pol = T.PointerHeadPolicy(scorer, greedy=True)
    return sp, scorer, pol, (static, dynamic, cs, n)


@pytest.mark.parametrize("D", [2, 3])
def test_lean_episode_equals_the_expanded_one(D):
    rows = 30 if D == 2 else 66
    enc, v = _encoder(rows, 32, 70 + D)
    res = {}
    for lean in (True, False):
        sp, scorer, pol, (static, dynamic, cs, n) = _episode(D, lean, enc, v)
        with torch.no_grad():
            sp.begin(static, dynamic)
            assert sp.dynamic_bits is not None and torch.equal(sp.dynamic_bits, pack.dynamic_bits(dynamic)[0])
            out = T.run_episode(static, dynamic, pol, cs[0], cs[-1], stepper=sp, check=False)
        assert (sp.dynamic is None) == lean
        res[lean] = (out["tour_idx"].clone(), pol.tour_logp().clone(), out["reward"].clone(), [h.cpu().numpy() for h in scorer.hidden])
    for a, b in zip(res[True][:3], res[False][:3]):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(res[True][1]).all())
    # at every step the hidden is the model applied to the oracle's dynamic
    tour = res[True][0].cpu().numpy()
    st, dyn = static.cpu().numpy(), dynamic.cpu().numpy()
    W, b = enc.conv.weight.detach().cpu().numpy()[:, :, 0], enc.conv.bias.detach().cpu().numpy()
    nR = dyn.shape[2]
    for t in range(n):
        want = M.encode(M.pack_bits(dyn), W, b, rows, nR)
        assert np.array_equal(res[True][3][t], want), t
        assert np.array_equal(res[False][3][t], want), t
        dyn = O.update_dynamic(dyn, st, tour[:, t], n, 3)


def test_dynamic_bits_before_step_0():
    n, static, dynamic, cs = _window(2)
    env = T.BatchedContainer(64, cs, n, "C+P+S-lb-soft", "diff", device=DEV)
    sp = T.EpisodeStepper(static, dynamic, env, 'bot', True, steps=n, expand_dynamic=False)
    want = pack.dynamic_bits(dynamic)[0]
    sp.begin(static, dynamic)
    assert torch.equal(sp.dynamic_bits, want)
    sp.step(torch.zeros(64, dtype=torch.int64, device=DEV))
    sp.begin(static, dynamic, initial_mask=False)
    assert sp.dynamic_bits is None                                # no launch built a shadow: not the previous episode's buffer
    mine = want.clone()
    sp.begin_shadow(static, dynamic, mine)
    assert sp.dynamic_bits is mine


def test_lean_episode_replays_from_a_hip_graph():
    """the lean episode (no fp32 dynamic anywhere) captured once -- linear, one stream -- and replayed with refreshed
    encoder weights: tour, tour_logp and reward equal the eager run's"""
    enc, v = _encoder(30, 32, 81)
    sp, scorer, pol, (static, dynamic, cs, n) = _episode(2, True, enc, v, keep=False)
    pack.set_binary_check('trust')
    try:
        def run():
            with torch.no_grad():
                out = T.run_episode(static, dynamic, pol, cs[0], cs[-1], stepper=sp, check=False)
                return out["tour_idx"], out["reward"], pol.tour_logp()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = run()
        tours = []
        for seed in (82, 83):
            fresh, _ = _encoder(30, 32, seed)
            with torch.no_grad():
                enc.conv.weight.copy_(fresh.conv.weight * 3)
                enc.conv.bias.copy_(fresh.conv.bias)
            graph.replay()
            torch.cuda.synchronize()
            got = [r.clone() for r in rec]
            eager = run()
            for a, b in zip(got, eager):
                assert torch.equal(a, b)
            tours.append(got[0].cpu().numpy())
        assert not np.array_equal(tours[0], tours[1])
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
