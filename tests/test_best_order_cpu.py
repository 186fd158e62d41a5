"""The greedy best-ratio order without a GPU: the fixture the reference wrote (generate_order_graph(..., 'best'),
tests/golden/best_order.npz) against a greedy loop built only from the oracle's initial_mask / update_dynamic /
update_mask and fresh oracle containers -- this pins the rule (current_mask in column order is the reference's valid
set; the first strict fp64 maximum wins) independently of the GPU -- and the host side of the new entry point."""
import inspect

import numpy as np
import pytest

import best_order_cases as BC
import tap_net_amd as T
from tap_net_amd import _lib, generate, rollout


def test_fixture_covers_what_it_should():
    cs = BC.CASES
    assert 50 <= len(cs) <= 70
    shapes = {(tuple(c.initial), tuple(c.target), c.n) for c in cs}
    for init, tgt in (((5, 50), (5, 50)), ((7, 50), (5, 50)), ((5, 5, 50), (5, 5, 50))):
        for n in (6, 10):
            assert (init, tgt, n) in shapes
    rts = {c.reward_type for c in cs}
    assert {"C+P+S-lb-soft", "C+P+S-lb-hard", "C+P+S-mcs-soft", "C+P+S-mul-soft"} <= rts
    assert sum(not c.allow_bot for c in cs) >= 3
    for c in cs:
        assert sorted(s % c.n for s in c.solution) == list(range(c.n))


@pytest.mark.parametrize("case", BC.CASES, ids=lambda c: c.id)
def test_oracle_greedy_reproduces_the_reference(case):
    solution, mean_valid, _ = BC.greedy(case)
    assert solution == case.solution
    assert abs(mean_valid - case.mean_valid) <= 1e-12


def test_ties_are_common():
    """a third of the reference's steps have an exact fp64 tie for the maximum: the pick has to be a first maximum"""
    rows = tied = 0
    for case in BC.CASES[:24]:
        for cur, scores in BC.greedy(case)[2]:
            rows += 1
            tied += int((scores == scores.max()).sum() > 1)
    assert tied * 4 >= rows, (tied, rows)


def test_entry_point_is_bound():
    assert "tap_env_trial_scores" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "tap_env_trial_scores")
    assert list(inspect.signature(T.BatchedContainer.trial_scores).parameters) == [
        "self", "static", "mask", "fresh", "out", "best_out", "stepped"]
    assert list(inspect.signature(generate.generate_order_graph).parameters) == [
        "blocks", "positions", "container_size", "arm_size", "allow_bot", "find_order_type", "reward_type",
        "target_container_size"]                                                           # generate.py:1109
    assert list(inspect.signature(generate.best_orders).parameters) == [
        "blocks", "positions", "initial_container_size", "target_container_size", "reward_type", "arm_size", "allow_bot"]
    assert T.BestRatioPolicy is rollout.BestRatioPolicy


@pytest.mark.parametrize("kind", ["rand", "max"])
def test_random_order_types_are_refused(kind):
    c = BC.CASES[0]
    with pytest.raises(NotImplementedError, match="numpy"):
        generate.generate_order_graph(c.blocks, c.positions, c.initial, 1, True, kind, c.reward_type, c.target)
    with pytest.raises(ValueError):
        generate.generate_order_graph(c.blocks, c.positions, c.initial, 1, True, "nope", c.reward_type, c.target)


def test_host_side_refusals_need_no_device():
    """the descriptor checks of the C entry run before anything touches the device"""
    import ctypes as C
    L = _lib.lib()
    d = _lib.make_desc(4, [5, 50], 10, "C+P+S-lb-soft", "full", "LB_GREEDY")
    assert L.tap_env_trial_scores(None, None, None, None, 3, 20, None, 0, None, None, None) == _lib.TAP_E_INVALID
    _lib.set_place_at(d, 'net')
    assert L.tap_env_trial_scores(None, C.byref(d), None, None, 3, 20, None, 0, None, None, None) == _lib.TAP_E_INVALID
    for cs, rt, strat in (([5, 50], "C+P+S-mcs-soft", "LB_GREEDY"), ([5, 50], "C+P+S-lb-soft", "LB"),
                          ([65, 50], "C+P+S-lb-soft", "LB_GREEDY"), ([9, 5, 50], "C+P+S-lb-soft", "LB_GREEDY")):
        d = _lib.make_desc(4, cs, 10, rt, "full", strat)
        assert L.tap_env_trial_scores(None, C.byref(d), None, None, 4, 20, None, 0, None, None, None) == _lib.TAP_E_UNSUPPORTED
    d = _lib.make_desc(0, [5, 50], 10, "C+P+S-lb-soft", "full", "LB_GREEDY")
    assert L.tap_env_trial_scores(None, C.byref(d), None, None, 3, 20, None, 0, None, None, None) == _lib.TAP_OK
    d = _lib.make_desc(4, [5, 50], 10, "C+P+S-lb-soft", "full", "LB_GREEDY")
    assert L.tap_env_trial_scores(None, C.byref(d), None, None, 3, 20, None, 4, None, None, None) == _lib.TAP_E_INVALID
    assert L.tap_env_trial_scores(None, C.byref(d), None, None, 3, 20, None, 0, None, None, None) == _lib.TAP_E_INVALID
