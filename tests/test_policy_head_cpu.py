"""The decoding head without a GPU: the exports and signatures, the C entries' host-side checks, and the numpy model
(tests/policy_head_model.py) against torch on the CPU, against its own sampling law, and against the condition the GPU
comparison relies on: no fixed u * S comes near a prefix sum."""
import ctypes as C
import inspect

import numpy as np
import torch
import torch.nn.functional as F

import policy_head_model as M
import tap_net_amd as T
from tap_net_amd import _lib


def test_exports_and_signatures():
    L = _lib.lib()
    for name in ("tap_policy_pick", "tap_policy_pick_backward"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.tap_abi_version() == 1
    assert list(inspect.signature(T.pointer_pick).parameters) == ["logits", "mask", "u", "want_probs"]
    sig = inspect.signature(T.pointer_pick).parameters
    assert sig["u"].default is None and sig["want_probs"].default is False
    assert list(inspect.signature(T.PointerHeadPolicy.__init__).parameters) == ["self", "scorer", "u", "greedy", "generator"]
    for meth in ("__call__", "tour_logp", "reset"):
        assert callable(getattr(T.PointerHeadPolicy, meth))
    assert T.rollout.pointer_pick is T.pointer_pick and "PointerHeadPolicy" in T.__all__ and "pointer_pick" in T.__all__
    assert _lib.TAP_HIT_POLICY_PICK == 26 and _lib.TAP_P_GREEDY == 1


def test_host_side_checks_need_no_device():
    """the argument checks of both entries, in the header's order, with a null context and null buffers"""
    L = _lib.lib()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    inv, ok = _lib.TAP_E_INVALID, _lib.TAP_OK
    # 1. B < 0 or nR < 1, before anything else
    assert L.tap_policy_pick(None, None, None, None, -1, 4, 0, None, None, None, None) == inv
    assert L.tap_policy_pick(None, None, None, None, 2, 0, 0, None, None, None, None) == inv
    assert L.tap_policy_pick(None, None, None, None, 0, 0, 0, None, None, None, None) == inv
    # 2. an empty batch is fine whatever the buffers and the flags are
    assert L.tap_policy_pick(None, None, None, None, 0, 4, 0, None, None, None, None) == ok
    assert L.tap_policy_pick(None, None, None, None, 0, 4, 6, None, None, None, None) == ok
    # 3. a null logits, mask, ptr_out or logp_out
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert L.tap_policy_pick(None, args[0], args[1], p, 1, 4, 0, args[2], args[3], None, None) == inv
    # 4. greedy with uniforms; sampling without
    assert L.tap_policy_pick(None, p, p, p, 1, 4, _lib.TAP_P_GREEDY, p, p, None, None) == inv
    assert L.tap_policy_pick(None, p, p, None, 1, 4, 0, p, p, None, None) == inv
    # 5. unknown flag bits
    assert L.tap_policy_pick(None, p, p, p, 1, 4, 2, p, p, None, None) == inv
    assert L.tap_policy_pick(None, p, p, None, 1, 4, _lib.TAP_P_GREEDY | 4, p, p, None, None) == inv
    # the backward
    assert L.tap_policy_pick_backward(None, None, None, None, None, -1, 4, None, None) == inv
    assert L.tap_policy_pick_backward(None, None, None, None, None, 1, 0, None, None) == inv
    assert L.tap_policy_pick_backward(None, None, None, None, None, 0, 4, None, None) == ok
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        assert L.tap_policy_pick_backward(None, args[0], args[1], args[2], args[3], 1, 4, args[4], None) == inv


def test_greedy_branch_is_torch_softmax_max():
    """0 / 1 masks with finite logits: the model's greedy branch = F.softmax(logits + mask.log()).max(1) and .log()"""
    for nR in (1, 7, 20, 65):
        rng = np.random.RandomState(nR)
        logits = (rng.randn(50, nR) * 3).astype(np.float32)
        mask = (rng.rand(50, nR) < 0.4).astype(np.float32)
        mask[mask.sum(1) == 0, nR // 2] = 1                       # torch's softmax of an all -inf row is NaN: not this test's
        logits[3, :] = 2.0                                        # a row of ties: the first selectable column
        mask[3, -2:] = 1
        ptr, logp, probs, _ = M.pick(logits, mask)
        want = F.softmax(torch.from_numpy(logits).double() + torch.from_numpy(mask).double().log(), 1)
        prob, tptr = want.max(1)
        w = want.numpy()
        assert np.array_equal(ptr, w.argmax(1))                   # numpy's argmax: the first maximum
        unique = (w == w.max(1, keepdims=True)).sum(1) == 1       # torch.max names no tie rule: compared where there is no tie
        assert (nR == 1 or not unique[3]) and np.array_equal(ptr[unique], tptr.numpy()[unique])
        assert np.abs(logp - prob.log().numpy()).max() <= 1e-12
        assert np.abs(probs - want.numpy()).max() <= 1e-14
        assert (probs[mask == 0] == 0).all()


def test_sampling_law_intervals():
    """for a fixed row the u mapped to column c form an interval of length p_c: its ends are the prefix sums / S"""
    rng = np.random.RandomState(7)
    logits = (rng.randn(12) * 3).astype(np.float32)
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0], np.float32)
    sel, m, w, cum, S = M.row_weights(logits, mask)
    _, _, probs, _ = M.pick_row(logits, mask)
    lo = 0.0
    for i, c in enumerate(sel):
        hi = cum[i] / S
        assert abs((hi - lo) - probs[c]) <= 1e-15
        # strictly inside the interval -> c; u is fp32, so step in by a few fp32 spacings
        inside = [lo + (hi - lo) * f for f in (0.01, 0.5, 0.99)]
        for x in inside:
            x32 = np.float32(x)
            if lo < float(x32) < hi and min(float(x32) - lo, hi - float(x32)) > 1e-7:
                assert M.pick_row(logits, mask, x32)[0] == c
        lo = hi
    assert abs(lo - 1.0) <= 1e-15
    assert abs(sum(probs) - 1.0) <= 1e-14 and (probs[mask == 0] == 0).all()
    # the ends of the range: u = 0 -> the first selectable column, the largest fp32 below 1 -> the last one here
    assert M.pick_row(logits, mask, np.float32(0.0))[0] == sel[0]
    assert M.pick_row(logits, mask, np.nextafter(np.float32(1.0), np.float32(0.0)))[0] == sel[-1]


def test_strict_rule_on_four_equal_logits():
    logits, mask = np.zeros(4, np.float32), np.ones(4, np.float32)
    for u, c in ((0.0, 0), (0.25, 1), (0.5, 2), (0.75, 3)):
        ptr, logp, probs, gap = M.pick_row(logits, mask, np.float32(u))
        assert ptr == c and logp == np.log(0.25) and (probs == 0.25).all()


def test_rules_at_the_edges():
    nan, inf = float('nan'), float('inf')
    # an empty row: ptr 0, logp NaN, probs 0 -- and no gradient
    ptr, logp, probs, _ = M.pick_row(np.array([1.0, 2.0], np.float32), np.zeros(2, np.float32), np.float32(0.3))
    assert ptr == 0 and np.isnan(logp) and (probs == 0).all()
    assert (M.backward(probs[None], np.array([0]), np.array([logp]), np.array([3.0])) == 0).all()
    # unselectable logits are never used, whatever they hold
    clean = M.pick_row(np.array([0.5, 0.0, -1.0, 0.0], np.float32), np.array([1, 0, 1, 0], np.float32), np.float32(0.9))
    for junk in (nan, inf, -inf):
        got = M.pick_row(np.array([0.5, junk, -1.0, junk], np.float32), np.array([1, 0, 1, 0], np.float32), np.float32(0.9))
        assert got[0] == clean[0] == 2 and got[1] == clean[1] and np.array_equal(got[2], clean[2])
    # one selectable column: that column for any u, logp exactly 0, probs exactly 1
    for u in (0.0, 0.5, np.nextafter(np.float32(1.0), np.float32(0.0))):
        ptr, logp, probs, _ = M.pick_row(np.array([3.0, -7.0, 80.0], np.float32), np.array([0, 1, 0], np.float32), np.float32(u))
        assert ptr == 1 and logp == 0.0 and probs[1] == 1.0


def test_fixed_cases_stay_clear_of_every_prefix_sum():
    """what keeps the GPU comparison of ptr honest with NO row excluded: every u * S of its fixed cases is at least
    MIN_GAP * S away from every prefix sum, while the device's prefix sums differ from the model's by the order of an
    fp64 sum of nR <= 300 terms in [0, 1] (about 1e-14 * S)."""
    rows, smallest = 0, float('inf')
    for nR in M.NR_LIST:
        for case in M.fixed_cases(nR):
            gap = M.reference(case, greedy=False)[3]
            rows += len(gap)
            smallest = min(smallest, float(gap.min()))
    print("rows %d, smallest gap %.3g * S" % (rows, smallest))
    assert rows == 5 * sum(sum(M.batch_sizes(nR)) for nR in M.NR_LIST)
    assert smallest >= M.MIN_GAP, smallest
