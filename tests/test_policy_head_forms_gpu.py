"""The DRAW and GIVEN forms of the decoding head on the MI355X (policy.hip: k_policy_pick_form<G, FORM>,
k_policy_pick_wide_form<FORM>) at the smallest shapes that reach every instantiation: nR = 5, 12, 20, 40, 64 (G = 8, 16, 32,
64, 64), 65 and 130 (the chunked form with a ragged and a third chunk); B = 1, one more row than a workgroup holds, and 67;
rows fully selectable, with one selectable column and with none.

DRAW is held to the existing sampling launch byte for byte (``pointer_pick(logits, mask, u_out)``) and its uniform to the
torch Philox; GIVEN to the bytes of the call whose pick it is given, and at arbitrary columns to the numpy fp64 model under
policy_head_model's neighbour rule."""
import numpy as np
import pytest
import torch

import policy_head_forms_model as FM
import policy_head_model as HM
import tap_net_amd as T
from tap_net_amd import _lib, rollout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, EPISODE, STEP, OFFSET = FM.DRAW_AT                        # the CPU test keeps these draws MIN_GAP off every prefix sum
DRAW, GIVEN = 2, 3                                              # the launch record's variant field


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _state(episode=EPISODE):
    return torch.tensor([SEED, episode], dtype=torch.int64, device=DEV)


def _bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype is torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype is torch.float32 else b)


def _keys():
    return {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_POLICY_PICK}


CASES = [(nR, B) for nR in FM.NR_LIST for B in FM.batch_sizes(nR)]


@pytest.mark.parametrize("nR,B", CASES)
def test_draw_is_the_sampling_launch_at_its_own_uniform(nR, B):
    """u_out is the torch Philox's uniform exactly (and the numpy model's); ptr, logp and probs are pointer_pick's bytes at
    u_out, with and without probs_out; ptr is the model's on every row; two calls give the same bytes; the launch record"""
    lg, mk = FM.case(nR, B)
    logits, mask, state = _dev(lg), _dev(mk), _state()
    _lib.variant_hits_reset(DEV)
    ptr, logp, probs, u = T.pointer_pick_draw(logits, mask, (state, STEP, OFFSET), want_probs=True, want_u=True)
    assert ptr.dtype is torch.int64 and logp.dtype is torch.float32 and u.dtype is torch.float32
    assert _bytes(u, rollout.pick_uniforms(state, STEP, B, OFFSET))
    assert np.array_equal(u.cpu().numpy(), FM.uniforms(SEED, EPISODE, STEP, B, OFFSET))
    want = T.pointer_pick(logits, mask, u, want_probs=True)
    for a, b in zip((ptr, logp, probs), want):
        assert _bytes(a, b)
    lean = T.pointer_pick_draw(logits, mask, rollout.PickRecord(state, STEP, OFFSET))
    assert len(lean) == 2 and _bytes(lean[0], ptr) and _bytes(lean[1], logp)
    again = T.pointer_pick_draw(logits, mask, (state, STEP, OFFSET), want_probs=True, want_u=True)
    for a, b in zip(again, (ptr, logp, probs, u)):
        assert _bytes(a, b)
    model = FM.draw(lg, mk, SEED, EPISODE, STEP, OFFSET)
    assert np.array_equal(ptr.cpu().numpy(), model[0]) and HM.neighbour32(logp.cpu().numpy(), model[1]).all()
    if B > 2:
        assert int(ptr[1]) == nR // 2 and float(logp[1]) == 0.0 and int(ptr[2]) == 0 and bool(torch.isnan(logp[2]))
        assert not bool(probs[2].any())
    G = HM.group_of(nR)
    assert {k for k in _keys() if k[3] == DRAW} == {(_lib.TAP_HIT_POLICY_PICK, 0, G, DRAW, p, 0, 0) for p in (0, 1)}


@pytest.mark.parametrize("nR,B", [c for c in CASES if c[1] > 1])
def test_draw_does_not_depend_on_how_the_batch_is_split(nR, B):
    """the batch in two calls, env_offset set for the second half: the bytes of the one call; another step, another episode
    and another offset each give other uniforms"""
    lg, mk = FM.case(nR, B)
    logits, mask, state = _dev(lg), _dev(mk), _state()
    whole = T.pointer_pick_draw(logits, mask, (state, STEP, OFFSET), want_probs=True, want_u=True)
    half = B // 2
    a = T.pointer_pick_draw(logits[:half], mask[:half], (state, STEP, OFFSET), want_probs=True, want_u=True)
    b = T.pointer_pick_draw(logits[half:], mask[half:], (state, STEP, OFFSET + half), want_probs=True, want_u=True)
    for w, x, y in zip(whole, a, b):
        assert _bytes(w, torch.cat((x, y), 0))
    for other in ((state, STEP + 1, OFFSET), (_state(EPISODE + 1), STEP, OFFSET), (state, STEP, OFFSET + 1)):
        assert not torch.equal(T.pointer_pick_draw(logits, mask, other, want_u=True)[2], whole[3])


@pytest.mark.parametrize("nR,B", CASES)
def test_given_at_the_picked_column_is_that_calls_bytes(nR, B):
    """the sampling and the greedy call's ptr fed back: their logp and probs, byte for byte; two calls agree; the record"""
    lg, mk = FM.case(nR, B)
    logits, mask = _dev(lg), _dev(mk)
    u = _dev(np.random.RandomState(nR + B).rand(B).astype(np.float32))
    _lib.variant_hits_reset(DEV)
    for uu in (u, None):
        ptr, logp, probs = T.pointer_pick(logits, mask, uu, want_probs=True)
        g_logp, g_probs = T.pointer_pick_given(logits, mask, ptr, want_probs=True)
        assert _bytes(g_logp, logp) and _bytes(g_probs, probs)
        assert _bytes(T.pointer_pick_given(logits, mask, ptr), logp)
    G = HM.group_of(nR)
    assert {k for k in _keys() if k[3] == GIVEN} == {(_lib.TAP_HIT_POLICY_PICK, 0, G, GIVEN, p, 0, 0) for p in (0, 1)}


@pytest.mark.parametrize("nR", FM.NR_LIST)
def test_given_at_arbitrary_columns_against_the_model(nR):
    """B = 67: a random column per row -- selectable, unselectable, -1 and nR among them --: logp and probs are the fp64
    model's value or an fp32 neighbour, NaN exactly where the model says (probs are written all the same); NaN and +-inf on
    the unselectable columns change no byte of either form"""
    B = 67
    lg, mk = FM.case(nR, B)
    rng = np.random.RandomState(31 + nR)
    cols = rng.randint(0, nR, size=B).astype(np.int64)
    cols[5], cols[6] = -1, nR
    want_logp, want_probs = FM.given(lg, mk, cols)
    assert np.isnan(want_logp[[2, 5, 6]]).all() and np.isfinite(want_logp).sum() > B // 4
    logp, probs = T.pointer_pick_given(_dev(lg), _dev(mk), _dev(cols), want_probs=True)
    assert HM.neighbour32(logp.cpu().numpy(), want_logp).all() and HM.neighbour32(probs.cpu().numpy(), want_probs).all()
    assert (probs.cpu().numpy()[mk == 0] == 0).all()
    state = _state()
    clean = T.pointer_pick_draw(_dev(lg), _dev(mk), (state, STEP, OFFSET), want_probs=True)
    for junk in (np.nan, np.inf, -np.inf):
        dirty = _dev(np.where(mk == 0, np.float32(junk), lg))
        got = T.pointer_pick_given(dirty, _dev(mk), _dev(cols), want_probs=True)
        assert _bytes(got[0], logp) and _bytes(got[1], probs)
        for a, b in zip(T.pointer_pick_draw(dirty, _dev(mk), (state, STEP, OFFSET), want_probs=True), clean):
            assert _bytes(a, b)


@pytest.mark.parametrize("nR", [12, 130])
def test_backward_is_the_heads_backward(nR):
    """autograd through both forms: dlogits is tap_policy_pick_backward's bytes for the same (probs, ptr, logp, g) -- what
    _PointerPick gives for pointer_pick at the same uniform; a NaN row (an out-of-range GIVEN column) has a zero gradient"""
    B = 67
    lg, mk = FM.case(nR, B)
    mask, state = _dev(mk), _state()
    g = _dev(np.random.RandomState(nR).randn(B).astype(np.float32))
    leaf = lambda: _dev(lg).requires_grad_(True)                                                               # noqa: E731
    _lib.variant_hits_reset(DEV)
    l_draw = leaf()
    ptr, logp, u = T.pointer_pick_draw(l_draw, mask, (state, STEP, OFFSET), want_u=True)
    assert logp.requires_grad and not ptr.requires_grad and not u.requires_grad
    logp.backward(g)
    l_ref = leaf()
    ptr_ref, logp_ref = T.pointer_pick(l_ref, mask, u)
    logp_ref.backward(g)
    assert _bytes(ptr, ptr_ref) and _bytes(l_draw.grad, l_ref.grad) and float(l_ref.grad.abs().max()) > 0
    l_given = leaf()
    T.pointer_pick_given(l_given, mask, ptr).backward(g)
    assert _bytes(l_given.grad, l_ref.grad)
    bad = ptr.clone()
    bad[0] = nR
    l_bad = leaf()
    lp = T.pointer_pick_given(l_bad, mask, bad)
    lp.backward(g)
    assert bool(torch.isnan(lp[0])) and not bool(l_bad.grad[0].any()) and _bytes(l_bad.grad[1:], l_ref.grad[1:])
    back = sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == _lib.TAP_HIT_POLICY_PICK and k[5] == 1)
    assert back == 4


def test_argument_checks():
    """a state on another device, of another dtype or shape; a ptr of the wrong shape; tensors off the GPU"""
    logits, mask = torch.zeros(3, 5, device=DEV), torch.ones(3, 5, device=DEV)
    with pytest.raises(ValueError):
        T.pointer_pick_draw(logits, mask, (torch.zeros(2, dtype=torch.int64), 0, 0))
    with pytest.raises(ValueError):
        T.pointer_pick_draw(logits, mask, (torch.zeros(2, dtype=torch.int32, device=DEV), 0, 0))
    with pytest.raises(ValueError):
        T.pointer_pick_draw(logits, mask, (torch.zeros(3, dtype=torch.int64, device=DEV), 0, 0))
    with pytest.raises(ValueError):
        T.pointer_pick_given(logits, mask, torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(T.TapError):
        T.pointer_pick_given(logits.cpu(), mask.cpu(), torch.zeros(3, dtype=torch.int64))
    L, c = _lib.lib(), _lib.ctx(DEV)
    out = torch.empty(3, device=DEV)
    assert L.tap_policy_pick_draw(c, _lib.ptr(logits), _lib.ptr(mask), None, 0, 0, 3, 5, _lib.ptr(torch.empty(3, dtype=torch.int64, device=DEV)),
                                  _lib.ptr(out), None, None, _lib.stream_of(torch.device(DEV))) == _lib.TAP_E_INVALID
    assert L.tap_policy_pick_given(c, _lib.ptr(logits), _lib.ptr(mask), None, 3, 5, _lib.ptr(out), None,
                                   _lib.stream_of(torch.device(DEV))) == _lib.TAP_E_INVALID


def test_a_step_dropout_feeds_the_policy():
    """PointerHeadPolicy.from_source: step k of an episode draws at the source's pick k; next_episode() draws anew"""
    lg, mk = FM.case(20, 67)
    logits, mask = _dev(lg), _dev(mk)
    sd = T.StepDropout(SEED, DEV, env_offset=OFFSET)
    pol = T.PointerHeadPolicy.from_source(lambda **kw: logits, sd)
    sd.next_episode()
    picks = [pol(step=k, current_mask=mask) for k in range(3)]
    assert sd.pick == 3 and sd.step == 0 and tuple(pol.tour_logp().shape) == (67, 3)
    for k in range(3):
        want = T.pointer_pick_draw(logits, mask, (sd.state, k, OFFSET))
        assert _bytes(picks[k], want[0]) and _bytes(pol.tour_logp()[:, k].contiguous(), want[1])
    assert np.array_equal(picks[2].cpu().numpy(), FM.draw(lg, mk, SEED, 1, 2, OFFSET)[0])
