"""The decoding head on the MI355X (policy.hip: k_policy_pick<G, GREEDY>, k_policy_pick_wide, k_policy_pick_backward)
against the sequential fp64 model of tests/policy_head_model.py.

``ptr`` is compared on EVERY row: the fixed cases keep every u * S at least MIN_GAP * S away from every prefix sum
(tests/test_policy_head_cpu.py checks exactly these cases; the cases made here assert the same condition on the host
before they compare), and the device's fp64 prefix sums differ from the model's only by the order of the sum.
``logp`` and ``probs`` are the model's fp64 value rounded to fp32 or an fp32 neighbour of it (the device's exp and log
differ from the host's in the last bits); probs is exactly 0 on unselectable columns and its rows sum to 1 within
nR * 2^-24."""
import numpy as np
import pytest
import torch

import policy_head_model as M
import tap_net_amd as T
from tap_net_amd import _lib, pack, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U_TOP = np.nextafter(np.float32(1.0), np.float32(0.0))            # the largest fp32 below 1


def _head(logits, mask, u=None, want_probs=True):
    """pointer_pick on numpy inputs -> numpy (ptr, logp[, probs])"""
    out = T.pointer_pick(torch.from_numpy(logits).to(DEV), torch.from_numpy(mask).to(DEV),
                         None if u is None else torch.from_numpy(u).to(DEV), want_probs=want_probs)
    return tuple(o.cpu().numpy() for o in out)


def _keys():
    return {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_POLICY_PICK}


def _compare(got, want, mask, what):
    ptr, logp, probs, _ = want
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32
    assert np.array_equal(got[0], ptr), (what, np.flatnonzero(got[0] != ptr)[:8])
    ok = M.neighbour32(got[1], logp)
    assert ok.all(), (what, got[1][~ok][:4], logp[~ok][:4])
    if len(got) > 2:
        nR = mask.shape[1]
        ok = M.neighbour32(got[2], probs)
        assert ok.all(), (what, got[2][~ok][:4], probs[~ok][:4])
        assert (got[2][mask == 0] == 0).all(), what
        live = mask.any(axis=1)
        assert (np.abs(got[2][live].astype(np.float64).sum(1) - 1.0) <= nR * 2.0 ** -24).all(), what
        assert (got[2][~live] == 0).all(), what


@pytest.mark.parametrize("nR", M.NR_LIST)
def test_head_against_model(nR):
    """every fixed case of this nR (B = 1, 3, 64 / G + 1, 257; randn * 3, +-80, all-equal logits; masks 13 %, 30 % and
    fully selectable, empty rows included), sample and greedy, with and without probs_out, and the launch record"""
    G = M.group_of(nR)
    _lib.variant_hits_reset(DEV)
    for case in M.fixed_cases(nR):
        logits, mask, u = M.sample_case(*case)
        for greedy in (False, True):
            want = M.reference(case, greedy)
            if not greedy:
                assert want[3].min() >= M.MIN_GAP
            for want_probs in (True, False):
                got = _head(logits, mask, None if greedy else u, want_probs)
                assert len(got) == (3 if want_probs else 2)
                _compare(got, want, mask, (case, greedy, want_probs))
    keys = _keys()
    assert keys == {(_lib.TAP_HIT_POLICY_PICK, 0, G, g, p, 0, 0) for g in (0, 1) for p in (0, 1)}, keys


def test_every_form_runs():
    """all four lane groups and the chunked form, by the launch record"""
    _lib.variant_hits_reset(DEV)
    for nR in (8, 9, 32, 33, 65):
        _head(np.zeros((3, nR), np.float32), np.ones((3, nR), np.float32), np.full(3, 0.5, np.float32), False)
    assert {k[2] for k in _keys()} == {8, 16, 32, 64, 0}


@pytest.mark.parametrize("nR", M.NR_LIST)
def test_single_and_empty_rows_and_the_ends_of_u(nR):
    """rows holding exactly one selectable column (the first, the last, a middle one): ptr is that column for any u,
    logp == 0.0 and probs == 1.0 exactly; rows holding none: ptr 0, logp NaN, probs 0; and u = 0.0 / the largest fp32
    below 1 on ordinary rows"""
    rng = np.random.RandomState(nR)
    B = 3 * 6 + 8
    logits = (rng.randn(B, nR) * 3).astype(np.float32)
    mask = np.zeros((B, nR), np.float32)
    only = np.array([0, nR - 1, nR // 2] * 6)
    mask[np.arange(18), only] = 1
    u = np.concatenate([np.repeat(np.array([0.0, U_TOP, 0.37], np.float32), 6), rng.rand(8).astype(np.float32)])
    u[18:22] = [0.0, U_TOP, 0.0, U_TOP]
    mask[20:24] = (rng.rand(4, nR) < 0.5)                            # rows 18, 19: empty; 20 .. 23: ordinary
    mask[20:24, rng.randint(nR)] = 1
    mask[24:] = 1
    u[24:26] = [0.0, U_TOP]
    want = M.pick(logits, mask, u)
    assert want[3][u != 0].min() >= M.MIN_GAP                        # (u = 0: every prefix sum is > 0 on both sides, exactly)
    for greedy in (False, True):
        got = _head(logits, mask, None if greedy else u)
        _compare(got, M.pick(logits, mask) if greedy else want, mask, greedy)
        assert np.array_equal(got[0][:18], only)
        assert (got[1][:18] == 0.0).all() and (got[2][np.arange(18), only] == 1.0).all()
        assert (got[0][18:20] == 0).all() and np.isnan(got[1][18:20]).all() and (got[2][18:20] == 0).all()


@pytest.mark.parametrize("nR", [7, 20, 60, 65, 300])
def test_unselectable_logits_are_never_used(nR):
    """NaN, +inf and -inf on the unselectable columns: every output bit for bit what the clean run gives"""
    case = M.fixed_cases(nR)[-5]                                    # B = 257, randn, 30 %
    logits, mask, u = M.sample_case(*case)
    assert case[1] == 257 and (mask == 0).any()
    for greedy in (False, True):
        clean = _head(logits, mask, None if greedy else u)
        for junk in (np.nan, np.inf, -np.inf):
            dirty = np.where(mask == 0, np.float32(junk), logits)
            got = _head(dirty, mask, None if greedy else u)
            assert np.array_equal(got[0], clean[0])
            for a, b in zip(got[1:], clean[1:]):
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), (greedy, junk)


def test_strict_rule_on_the_device():
    """four equal logits, u = 0, .25, .5, .75 -> columns 0, 1, 2, 3 (cum > t is strict); all-equal logits under the
    greedy branch take the first selectable column"""
    u = np.array([0.0, 0.25, 0.5, 0.75], np.float32)
    ptr, logp, probs = _head(np.zeros((4, 4), np.float32), np.ones((4, 4), np.float32), u)
    assert ptr.tolist() == [0, 1, 2, 3] and (probs == 0.25).all() and M.neighbour32(logp, np.full(4, np.log(0.25))).all()
    mask = np.array([[0, 0, 1, 1], [0, 1, 0, 1], [1, 1, 1, 1], [0, 0, 0, 1]], np.float32)
    assert _head(np.full((4, 4), -3.25, np.float32), mask)[0].tolist() == [2, 1, 0, 3]


@pytest.mark.parametrize("nR", [20, 120])
def test_stratified_counts(nR):
    """4 096 rows of ONE logits / mask row with u = (i + 0.5) / 4096: the per-column counts are the model's, exactly"""
    rng = np.random.RandomState(5 + nR)
    n = 4096
    row, mrow = (rng.randn(nR) * 3).astype(np.float32), (rng.rand(nR) < 0.3).astype(np.float32)
    assert mrow.sum() >= 3
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    sel, m, w, cum, S = M.row_weights(row, mrow)
    t = u.astype(np.float64) * S
    assert np.abs(t[:, None] - np.asarray(cum)[None, :]).min() / S >= M.MIN_GAP
    want = np.asarray(sel)[np.minimum((t[:, None] >= np.asarray(cum)[None, :]).sum(1), len(sel) - 1)]
    assert want[7] == M.pick_row(row, mrow, u[7])[0] and want[-1] == M.pick_row(row, mrow, u[-1])[0]
    ptr, logp = _head(np.tile(row, (n, 1)), np.tile(mrow, (n, 1)), u, want_probs=False)
    assert np.array_equal(np.bincount(ptr, minlength=nR), np.bincount(want, minlength=nR))
    assert np.array_equal(ptr, want)
    assert np.abs(np.bincount(ptr, minlength=nR) / n - M.pick_row(row, mrow)[2]).max() <= 1.0 / n


@pytest.mark.parametrize("nR", [7, 20, 64, 65, 300])
def test_backward_against_torch_autograd(nR):
    """pointer_pick under autograd with a random g against torch's own autograd of log_softmax(logits + log(mask))[ptr]
    in fp64 on the CPU: every element within 2^-22 * |g_b| (two fp32 roundings of values bounded by |g_b|), exactly 0
    on unselectable columns and on empty rows -- also with NaN on the unselectable logits"""
    B = 257
    rng = np.random.RandomState(40 + nR)
    logits = (rng.randn(B, nR) * 3).astype(np.float32)
    mask = (rng.rand(B, nR) < 0.3).astype(np.float32)
    mask[5] = 0
    mask[6] = 1
    u, g = rng.rand(B).astype(np.float32), rng.randn(B).astype(np.float32)
    live = mask.any(axis=1)
    assert (~live).any() and M.pick(logits, mask, u)[3].min() >= M.MIN_GAP
    for poison in (False, True):
        for uu in (u, None):
            x = torch.from_numpy(np.where(mask == 0, np.float32(np.nan), logits) if poison else logits).to(DEV).requires_grad_()
            _lib.variant_hits_reset(DEV)
            ptr, logp = T.pointer_pick(x, torch.from_numpy(mask).to(DEV), None if uu is None else torch.from_numpy(uu).to(DEV))
            assert logp.requires_grad and not ptr.requires_grad
            logp.backward(torch.from_numpy(g).to(DEV))
            assert _keys() == {(26, 0, M.group_of(nR), 0 if uu is not None else 1, 1, 0, 0), (26, 0, 0, 0, 0, 1, 0)}
            got = x.grad.cpu().numpy()
            ptr = ptr.cpu().numpy()
            assert np.array_equal(ptr, M.pick(logits, mask, uu)[0])
            ref = torch.from_numpy(logits[live]).double().requires_grad_()
            lsm = torch.log_softmax(ref + torch.from_numpy(mask[live]).double().log(), 1)
            lsm.gather(1, torch.from_numpy(ptr[live]).view(-1, 1)).squeeze(1).backward(torch.from_numpy(g[live]).double())
            want = np.zeros((B, nR))
            want[live] = ref.grad.numpy()
            assert (np.abs(got - want) <= 2.0 ** -22 * np.abs(g)[:, None]).all(), np.abs(got - want).max()
            assert (got[mask == 0] == 0).all() and (got[~live] == 0).all()
            # a row sums to zero within the ONE rounding of its picked column, as the true gradient does: that column is
            # minus the fp64 sum of the others (whose own error, <= nR additions of 2^-53, is far below)
            picked = np.abs(got[np.arange(B), ptr].astype(np.float64))
            assert (np.abs(got.astype(np.float64).sum(1)) <= 2.0 ** -24 * picked + 2.0 ** -45 * np.abs(g)).all()
    # the forward is the same without grad; half logits come back as a half gradient (autograd handles the cast)
    with torch.no_grad():
        assert not T.pointer_pick(x, torch.from_numpy(mask).to(DEV))[1].requires_grad
    h = torch.from_numpy(logits).to(DEV).half().requires_grad_()
    T.pointer_pick(h, torch.from_numpy(mask).to(DEV))[1].nan_to_num(0.0).sum().backward()
    assert h.grad.dtype is torch.float16 and bool(torch.isfinite(h.grad).all())


# ---- the head in the decoding loop ----------------------------------------------------------------------------------
B_LOOP, N_LOOP = 64, 10


class _Scorer(object):
    """a fixed random projection of decoder_dynamic plus a per-column bias (element-wise ops only: nothing here
    synchronises or needs a library workspace, so the episode can be captured); keeps what the head was given"""

    def __init__(self, flen, nR, seed, keep=True):
        rng = np.random.RandomState(seed)
        self.P = torch.from_numpy(rng.randn(1, flen, nR).astype(np.float32)).to(DEV)
        self.bias = torch.from_numpy((rng.randn(1, nR) * 2).astype(np.float32)).to(DEV)
        self.keep, self.logits, self.masks = keep, [], []

    def __call__(self, step, current_mask, decoder_dynamic, **_):
        B = current_mask.shape[0]
        logits = (decoder_dynamic.reshape(B, -1, 1) * 0.05 * self.P).sum(1) + self.bias
        if self.keep:
            self.logits.append(logits.clone())
            self.masks.append(current_mask.clone())
        return logits


def _loop_instances(seed):
    return synth.rand_instances(B_LOOP, N_LOOP, 2, seed=seed)


def _check_episode(out, pol, scorer, u):
    tour = out["tour_idx"].cpu().numpy()
    logp = pol.tour_logp().cpu().numpy()
    assert tour.shape == logp.shape == (B_LOOP, N_LOOP)
    for t in range(N_LOOP):
        mask, logits = scorer.masks[t].cpu().numpy(), scorer.logits[t].cpu().numpy()
        if t:
            assert np.array_equal(mask, out["current_masks"][t - 1].cpu().numpy())       # the recorded masks, one step on
        assert (mask[np.arange(B_LOOP), tour[:, t]] != 0).all(), t
        want = M.pick(logits, mask, u[t])
        assert want[3].min() >= M.MIN_GAP
        assert np.array_equal(tour[:, t], want[0]), t
        assert M.neighbour32(logp[:, t], want[1]).all(), t
    out["env"].check()


@pytest.mark.parametrize("fused", [True, False])
def test_policy_in_run_episode(fused):
    """run_episode at 2D W = 5, n = 10, B = 64 under PointerHeadPolicy with pre-drawn u, on the fused stepper and on the
    two-launch loop: every pick selectable under the mask the head saw and equal to the model's pick replayed from the
    recorded masks and logits, tour_logp() the model's, the containers clean"""
    static, dynamic = _loop_instances(31)
    u = np.random.RandomState(32).rand(N_LOOP, B_LOOP).astype(np.float32)
    scorer = _Scorer(4, 2 * N_LOOP, 33)
    pol = T.PointerHeadPolicy(scorer, u=torch.from_numpy(u).to(DEV))
    with torch.no_grad():
        out = T.run_episode(static.to(DEV), dynamic.to(DEV), pol, 5, 50, record=True, fused=fused)
    _check_episode(out, pol, scorer, u)
    # the greedy form and the eager draw: selectable picks, finite log-probabilities, a fresh tour_logp per episode
    for kw in (dict(greedy=True), dict(generator=torch.Generator(device=DEV).manual_seed(3))):
        s2 = _Scorer(4, 2 * N_LOOP, 33)
        p2 = T.PointerHeadPolicy(s2, **kw)
        with torch.no_grad():
            o2 = T.run_episode(static.to(DEV), dynamic.to(DEV), p2, 5, 50, fused=fused)
        tour = o2["tour_idx"].cpu().numpy()
        for t in range(N_LOOP):
            assert (s2.masks[t].cpu().numpy()[np.arange(B_LOOP), tour[:, t]] != 0).all()
        assert p2.tour_logp().shape == (B_LOOP, N_LOOP) and bool(torch.isfinite(p2.tour_logp()).all())
        if "greedy" in kw:
            assert np.array_equal(tour[:, 0], M.pick(s2.logits[0].cpu().numpy(), s2.masks[0].cpu().numpy())[0])
        p2.reset()
        with pytest.raises(RuntimeError):
            p2.tour_logp()
        o2["env"].check()


def test_episode_with_log_probabilities_replays_from_a_hip_graph():
    """the same episode captured once (linear, one stream, no grad) and replayed on two refreshed u buffers and
    instance sets: tour, reward and tour_logp equal the eager run's"""
    sets = [_loop_instances(seed) for seed in (41, 42, 43)]
    us = [np.random.RandomState(50 + i).rand(N_LOOP, B_LOOP).astype(np.float32) for i in range(3)]
    st, dy = sets[0][0].to(DEV), sets[0][1].to(DEV)
    u = torch.from_numpy(us[0]).to(DEV)
    env = T.BatchedContainer(B_LOOP, [5, 50], N_LOOP, "C+P+S-lb-soft", "diff", device=DEV)
    scorer = _Scorer(4, 2 * N_LOOP, 44, keep=False)
    pol = T.PointerHeadPolicy(scorer, u=u)
    pack.set_binary_check('trust')
    try:
        def run():
            with torch.no_grad():
                out = T.run_episode(st, dy.clone(), pol, 5, 50, env=env)
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
        for (static, dynamic), unew in zip(sets[1:], us[1:]):
            st.copy_(static)
            dy.copy_(dynamic)
            u.copy_(torch.from_numpy(unew))
            graph.replay()
            torch.cuda.synchronize()
            got = [r.clone() for r in rec]
            eager = run()
            for a, b in zip(got, eager):
                assert torch.equal(a, b)
            assert bool(torch.isfinite(got[2]).all())
            tours.append(got[0].cpu().numpy())
        assert not np.array_equal(tours[0], tours[1])
        env.check()
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
