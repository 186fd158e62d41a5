"""The DRAW and GIVEN forms of the decoding head without a GPU: the numpy model (tests/policy_head_forms_model.py) against
the package's torch forms (rollout.philox4x32_10, rollout.pick_uniforms, rollout.pointer_pick_torch) and against the
existing sampling model (tests/policy_head_model.py); the pick counter of tools.StepDropout."""
import numpy as np
import pytest
import torch

import policy_head_forms_model as FM
import policy_head_model as HM
import tap_net_amd as T
from tap_net_amd import rollout

SEEDS = [0, 0x1234567, (0x7EADBEEF << 32) | 0x9E3779B9]          # the key's high word zero and not


@pytest.mark.parametrize("seed", SEEDS)
def test_torch_and_numpy_philox_give_the_same_integers(seed):
    """the four output words at the pick's counter, torch integer ops against numpy uint64, and the uniform made of them;
    every u lies in [0, 1)"""
    for episode, step, off in ((0, 0, 0), (3, 9, 0), ((1 << 32) + 5, 41, 1000), (7, 2, 0xFFFFFFF0)):
        B = 40
        want = FM.words(seed, episode, step, np.arange(B, dtype=np.uint64) + np.uint64(off))
        env = (torch.arange(B, dtype=torch.int64) + off) & 0xFFFFFFFF
        zero = torch.zeros_like(env)
        got = rollout.philox4x32_10((env, zero + FM.PICK_ROW, zero + step, zero + (episode & 0xFFFFFFFF)),
                                    (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        for g, w in zip(got, want):
            assert np.array_equal(g.numpy().astype(np.uint64), w)
        state = torch.tensor([seed, episode], dtype=torch.int64)
        u = rollout.pick_uniforms(state, step, B, off)
        want_u = FM.uniforms(seed, episode, step, B, off)
        assert u.dtype is torch.float32 and np.array_equal(u.numpy().view(np.uint32), want_u.view(np.uint32))
        assert np.array_equal(want_u.astype(np.float64) * 2.0 ** 24, (want[0] >> np.uint64(8)).astype(np.float64))   # exact
        assert (want_u >= 0).all() and (want_u < 1).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_the_picks_row_is_none_of_the_dropout_rows(seed):
    """hidden row 0xFFFFFFFF against rows 0 .. 255 of the same (seed, episode, step, env): the output words differ (Philox is
    a bijection of the counter), so a pick never re-reads a dropout mask's draw"""
    for episode, step in ((0, 0), (5, 7)):
        envs = np.arange(8, dtype=np.uint64)
        pick = np.stack(FM.words(seed, episode, step, envs), axis=-1)                              # (8, 4)
        for row in range(256):
            other = np.stack(FM.words(seed, episode, step, envs, row=row), axis=-1)
            assert (pick != other).any(axis=-1).all(), row
            assert (pick[:, 0] != other[:, 0]).all(), row          # and word 0, the one both sides read, at these fixed seeds


@pytest.mark.parametrize("nR", FM.NR_LIST)
def test_draw_is_the_sampling_model_at_its_uniform(nR):
    """u fed to policy_head_model.pick: the DRAW model's ptr, logp and probs, bit for bit; u stays MIN_GAP away from every
    prefix sum, so the GPU test may compare ptr on every row"""
    for B in FM.batch_sizes(nR):
        logits, mask = FM.case(nR, B)
        ptr, logp, probs, u = FM.draw(logits, mask, *FM.DRAW_AT)
        want = HM.pick(logits, mask, u)
        assert np.array_equal(ptr, want[0]) and np.array_equal(logp.view(np.int64), want[1].view(np.int64))
        assert np.array_equal(probs, want[2])
        assert want[3].min() >= HM.MIN_GAP
        # an env's draw depends on its index in the whole batch alone
        if B > 1:
            half = B // 2
            tail = FM.draw(logits[half:], mask[half:], *FM.DRAW_AT[:3], FM.DRAW_AT[3] + half)
            assert np.array_equal(tail[0], ptr[half:]) and np.array_equal(tail[3], u[half:])


@pytest.mark.parametrize("nR", FM.NR_LIST)
def test_given_is_the_sampling_models_logp(nR):
    """at the sampling model's pick: its logp and probs bit for bit; NaN on an unselectable column and outside [0, nR), with
    probs still the row's"""
    B = FM.batch_sizes(nR)[-1]
    logits, mask = FM.case(nR, B)
    u = np.random.RandomState(nR).rand(B).astype(np.float32)
    for uu in (u, None):
        ptr, logp, probs, _ = HM.pick(logits, mask, uu)
        g_logp, g_probs = FM.given(logits, mask, ptr)
        assert np.array_equal(g_logp.view(np.int64), logp.view(np.int64)) and np.array_equal(g_probs, probs)
    assert not mask[2].any() and np.array_equal(np.isnan(logp), ~mask.any(axis=1))      # NaN on the empty rows alone
    bad = ptr.copy()
    rows = [b for b in range(B) if (mask[b] == 0).any() and mask[b].any()]
    for b in rows:
        bad[b] = int(np.flatnonzero(mask[b] == 0)[0])
    bad[0], bad[3] = nR, -1
    g_logp, g_probs = FM.given(logits, mask, bad)
    assert np.isnan(g_logp[rows + [0, 3]]).all() and np.array_equal(g_probs, probs)


@pytest.mark.parametrize("nR", [5, 40, 130])
def test_the_torch_head_is_the_model(nR):
    """rollout.pointer_pick_torch (tools.DRL's head off the GPU), float64: the models' ptr, logp within 1e-12, NaN where they
    say; its gradient is onehot - probs, zero on NaN rows"""
    B = 67
    lg, mk = FM.case(nR, B)
    logits, mask = torch.from_numpy(lg).double().requires_grad_(True), torch.from_numpy(mk)
    state = torch.tensor([11, 2], dtype=torch.int64)
    u = rollout.pick_uniforms(state, 3, B, 5)
    want = FM.draw(lg, mk, 11, 2, 3, env_offset=5)
    greedy = HM.pick(lg, mk)
    for got, ref in ((rollout.pointer_pick_torch(logits, mask, u), want), (rollout.pointer_pick_torch(logits, mask), greedy)):
        assert np.array_equal(got[0].numpy(), ref[0])
        assert np.array_equal(np.isnan(got[1].detach().numpy()), np.isnan(ref[1]))
        live = ~np.isnan(ref[1])
        assert np.abs(got[1].detach().numpy()[live] - ref[1][live]).max() <= 1e-12
    tour = torch.from_numpy(want[0]).clone()
    tour[0] = nR                                                 # out of range: NaN, no gradient
    ptr, logp = rollout.pointer_pick_torch(logits, mask, None, tour)
    g = torch.from_numpy(np.random.RandomState(1).randn(B))
    torch.where(torch.isnan(logp), torch.zeros_like(logp), logp * g).sum().backward()
    lp = logp.detach().numpy()
    dead = ~mk.any(axis=1)
    dead[0] = True
    assert dead[2] and np.array_equal(np.isnan(lp), dead)
    ref = HM.backward(want[2], want[0], np.where(dead, np.nan, want[1]), g.numpy())
    assert np.abs(logits.grad.numpy() - ref).max() <= 1e-12 and not logits.grad.numpy()[dead].any()


def test_take_pick_counts_on_its_own():
    """StepDropout.take_pick: (state, pick, env_offset), a counter beside the dropout step; next_episode resets both"""
    sd = T.StepDropout(9, "cpu", env_offset=64)
    a, s, b = sd.take_pick(), sd.take_step(0.1, 0.1), sd.take_pick()
    assert (a.step, b.step, s.step, sd.step, sd.pick) == (0, 1, 0, 1, 2)
    assert a.state is sd.state and a.env_offset == 64 and isinstance(a, rollout.PickRecord)
    sd.next_episode()
    assert (sd.step, sd.pick, sd.state.tolist()) == (0, 0, [9, 1])
    with pytest.raises(TypeError):
        T.PointerHeadPolicy.from_source(lambda **kw: None, torch.Generator())
    pol = T.PointerHeadPolicy.from_source(lambda **kw: None, sd)
    assert pol.source is sd and not pol.greedy and pol.u is None and T.PointerHeadPolicy(lambda **kw: None).source is None
    assert T.pointer_pick_draw is rollout.pointer_pick_draw and T.pointer_pick_given is rollout.pointer_pick_given
