"""The one-launch L-Pnet pick on the MI355X (dqn.hip: k_dqn_pick; tapenv.h: tap_dqn_pick) against the float64 model of
tests/dqn_pick_model.py, the same fold in float32 torch ops, and through its callers."""
import numpy as np
import pytest
import torch

import dqn_pick_model as DM
import pointer_model as PM
import tap_net_amd as T
from tap_net_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RT = 'C+P+S-SL-soft'
_shared = {}


def _te(case):
    return _lib.dqn_pick_geometry(*case)[0]


def _case(case):
    """per case, computed once and left unchanged: the fused net, 3 TE + 5 inputs, the float64 model's outputs on them, the
    stock float32 forward's (the reference whose error sets the tolerance) and the same fold's in float32 torch ops"""
    if case not in _shared:
        W, diff = case
        B = 3 * _te(case) + 5
        net = DM.seeded(W, diff, device=DEV, fused=True)
        hm, blk = (t.to(DEV) for t in DM.inputs(W, diff, B))
        net64 = DM.seeded(W, diff, device=DEV, dtype=torch.float64)
        with torch.no_grad():
            x64, logp64, probs64 = T.rollout.dqn_pick_torch(net64.fold(), hm.double(), blk.double(), want_probs=True)
            p32 = net(hm, blk)
            xf, logpf, probsf = T.rollout.dqn_pick_torch(net.fold(), hm, blk, want_probs=True)
        best = p32.max(1)
        _shared[case] = dict(net=net, hm=hm, blk=blk, x64=x64.cpu().numpy(), logp64=logp64.cpu().numpy(), probs64=probs64.cpu().numpy(),
                             e_logp=float((best[0].log().double() - logp64).abs().max()), e_probs=float((p32.double() - probs64).abs().max()),
                             x32=best[1].cpu().numpy(), xf=xf.cpu().numpy(), logpf=logpf.cpu().numpy(), probsf=probsf.cpu().numpy())
    return _shared[case]


def _hits():
    return {k: v for k, v in _lib.variant_hits(DEV).items() if k[0] == _lib.TAP_HIT_DQN}


def _key(case):
    te, P, _ = _lib.dqn_pick_geometry(*case)
    return (33, 2, te, 1 if case[1] else 0, P, 0, 0)


def _batches(case):
    te = _te(case)
    return [1, te - 1, te, te + 1, 3 * te + 5]


@pytest.mark.parametrize("case", DM.CASES, ids=DM.case_id)
def test_against_the_float64_model(case):
    c = _case(case)
    f = c['net'].fold()
    seen = set()
    for B in _batches(case):
        _lib.variant_hits_reset(DEV)
        x, logp, probs = T.rollout.dqn_pick(f, c['hm'][:B], c['blk'][:B], want_probs=True)
        assert _hits() == {_key(case): 1}
        assert x.dtype == torch.int64 and tuple(x.shape) == (B,) and tuple(probs.shape) == (B, case[0])
        x, logp, probs = x.cpu().numpy(), logp.cpu().numpy().astype(np.float64), probs.cpu().numpy().astype(np.float64)
        tl, tp = PM.tolerance(c['e_logp'], c['logp64'][:B]), PM.tolerance(c['e_probs'], c['probs64'][:B])
        dl, dp = np.abs(logp - c['logp64'][:B]).max(), np.abs(probs - c['probs64'][:B]).max()
        print("%s B %d: logp off by %.3g (tolerance %.3g, torch float32 %.3g), probs %.3g (%.3g, %.3g)"
              % (DM.case_id(case), B, dl, tl, c['e_logp'], dp, tp, c['e_probs']))
        assert dl <= tl and dp <= tp, (B, dl, tl, dp, tp)
        keep = DM.compared(c['probs64'][:B])
        assert np.array_equal(x[keep], c['x64'][:B][keep]), B
        seen |= set(x.tolist())
    if case[0] > 2:
        assert len(seen) >= 2, "a constant pick"


@pytest.mark.parametrize("case", DM.CASES, ids=DM.case_id)
def test_against_the_same_fold_in_float32(case):
    c = _case(case)
    B = len(c['x64'])
    x, logp, probs = T.rollout.dqn_pick(c['net'].fold(), c['hm'], c['blk'], want_probs=True)
    dl = np.abs(logp.cpu().numpy().astype(np.float64) - c['logpf']).max()
    dp = np.abs(probs.cpu().numpy().astype(np.float64) - c['probsf']).max()
    tl, tp = PM.tolerance(c['e_logp'], c['logp64']), PM.tolerance(c['e_probs'], c['probs64'])
    assert dl <= tl and dp <= tp, "B %d: logp off by %.3g (tolerance %.3g), probs by %.3g (%.3g)" % (B, dl, tl, dp, tp)
    keep = DM.compared(c['probs64'])
    assert np.array_equal(x.cpu().numpy()[keep], c['xf'][keep])
    print("observed maximum against the float32 fold: logp %.3g, probs %.3g" % (dl, dp))


@pytest.mark.parametrize("case", [(5, True), (9, True)], ids=DM.case_id)
def test_same_bytes(case):
    W, diff = case
    net = _case(case)['net']
    hm, blk = (t.to(DEV) for t in DM.inputs(W, diff, 37, seed=9))
    a = T.rollout.dqn_pick(net.fold(), hm, blk, want_probs=True)
    b = T.rollout.dqn_pick(net.fold(), hm, blk, want_probs=True)
    part = T.rollout.dqn_pick(net.fold(), hm[5:21], blk[5:21], want_probs=True)
    for u, v, w in zip(a, b, part):
        assert torch.equal(u, v)
        assert torch.equal(u[5:21], w)


def test_views_are_read_in_place():
    case = (5, True)
    c = _case(case)
    B, n, t = 37, 4, 2
    hm, blk = c['hm'][:B], c['blk'][:B]
    want = T.rollout.dqn_pick(c['net'].fold(), hm, blk, want_probs=True)
    blocks_f = torch.full((B, n, 2), 77.0, device=DEV)
    blocks_f[:, t] = blk[:, 0]
    view = blocks_f[:, t:t + 1, :]
    assert not view.is_contiguous() and T.rollout._dqn_view(view[:, 0])[0].data_ptr() == view.data_ptr()
    hm2 = hm.clone()
    hm2[:, :, -1] = 123.0                                                  # the diff form's trailing entry: never read
    got = T.rollout.dqn_pick(c['net'].fold(), hm2, view, want_probs=True)
    for u, v in zip(want, got):
        assert torch.equal(u, v)
    with torch.no_grad():
        x, logp = c['net'].pick(hm2, view)
    assert torch.equal(x, want[0]) and torch.equal(logp, want[1])


def _raw(w, pnet, ps, block, bs, B, x, logp, probs):
    ctx = _lib.ctx(DEV)
    return _lib.lib().tap_dqn_pick(ctx, _lib.C.byref(w), _lib.ptr(pnet), ps, _lib.ptr(block), bs, B, _lib.ptr(x), _lib.ptr(logp),
                                   _lib.ptr(probs), _lib.stream_of(torch.device(DEV)))


@pytest.mark.parametrize("want_probs", [True, False])
def test_canaries(want_probs):
    case = (5, False)
    c = _case(case)
    W, B, pad = 5, 19, 8
    hm, blk = c['hm'][:B, 0].contiguous(), c['blk'][:B, 0].contiguous()
    w = c['net'].fold().weights(torch.device(DEV))
    xb = torch.full((B + 2 * pad,), -7, dtype=torch.int64, device=DEV)
    lb = torch.full((B + 2 * pad,), -7.0, device=DEV)
    pb = torch.full((B * W + 2 * pad,), -7.0, device=DEV)
    assert _raw(w, hm, W, blk, 2, B, xb[pad:], lb[pad:], pb[pad:] if want_probs else None) == _lib.TAP_OK
    torch.cuda.synchronize()
    want = T.rollout.dqn_pick(c['net'].fold(), hm, blk, want_probs=True)
    assert torch.equal(xb[pad:pad + B], want[0]) and torch.equal(lb[pad:pad + B], want[1])
    for buf, n in ((xb, B), (lb, B), (pb, B * W)):
        assert bool((buf[:pad] == -7).all()) and bool((buf[pad + n:] == -7).all())
    if want_probs:
        assert torch.equal(pb[pad:pad + B * W].view(B, W), want[2])
    else:
        assert bool((pb == -7).all())


def test_launch_record_and_fallbacks():
    case = (5, True)
    c = _case(case)
    hm, blk = c['hm'][:9], c['blk'][:9]
    net = c['net']

    def stock(m, a=hm, b=blk):
        best = m(a, b).max(1)
        return best[1], best[0].log()
    _lib.variant_hits_reset(DEV)
    with torch.no_grad():
        x, logp = net.pick(hm, blk)
    assert _hits() == {_key(case): 1}
    assert tuple(x.shape) == (9,) and tuple(logp.shape) == (9,)
    _lib.variant_hits_reset(DEV)
    x, logp = net.pick(hm, blk)                                            # grad enabled, parameters that require one
    assert not _hits() and logp.requires_grad
    for u, v in zip((x, logp), stock(net)):
        assert torch.equal(u, v)
    with torch.no_grad():
        unfused = DM.seeded(5, True, device=DEV)
        for u, v in zip(unfused.pick(hm, blk), stock(unfused)):
            assert torch.equal(u, v)
        assert not _hits()
        training = DM.seeded(5, True, device=DEV, fused=True).train()      # (a forward in train() moves the running statistics)
        x, logp = training.pick(hm, blk)
        assert not _hits() and tuple(x.shape) == (9,)
        wide = DM.seeded(64, True, device=DEV, fused=True)
        h64, b64 = (t.to(DEV) for t in DM.inputs(64, True, 3))
        for u, v in zip(wide.pick(h64, b64), stock(wide, h64, b64)):
            assert torch.equal(u, v)
        assert not _hits()
    net.requires_grad_(False)
    try:
        _lib.variant_hits_reset(DEV)
        net.pick(hm, blk)                                                  # grad enabled, nothing requires one
        assert _hits() == {_key(case): 1}
    finally:
        net.requires_grad_(True)


def test_argument_checks():
    c = _case((5, True))
    f = c['net'].fold()
    w = f.weights(torch.device(DEV))
    B = 4
    hm, blk = c['hm'][:B, 0].contiguous(), c['blk'][:B, 0].contiguous()
    x = torch.zeros(B, dtype=torch.int64, device=DEV)
    logp = torch.zeros(B, device=DEV)
    assert _raw(w, hm, 5, blk, 2, B, x, logp, None) == _lib.TAP_OK
    bad = _lib.DqnWeights.from_buffer_copy(w)
    bad.L1p = w.L1p + 4                                                    # inside the buffer, not 16-byte aligned
    assert _raw(bad, hm, 5, blk, 2, B, x, logp, None) == _lib.TAP_E_INVALID
    bad = _lib.DqnWeights.from_buffer_copy(w)
    bad.W, bad.Wm, bad.P = 64, 63, 65
    assert _raw(bad, hm, 64, blk, 2, B, x, logp, None) == _lib.TAP_E_UNSUPPORTED   # refused before any read
    bad = _lib.DqnWeights.from_buffer_copy(w)
    bad.P = 7
    assert _raw(bad, hm, 5, blk, 2, B, x, logp, None) == _lib.TAP_E_INVALID
    assert _raw(w, hm, 3, blk, 2, B, x, logp, None) == _lib.TAP_E_INVALID   # an env stride shorter than the map
    assert _raw(w, hm, 5, blk, 2, 0, None, None, None) == _lib.TAP_OK
    wide = DM.seeded(64, True, device=DEV, fused=True)
    with pytest.raises(_lib.TapError) as e:
        T.rollout.dqn_pick(wide.fold(), torch.zeros(2, 1, 64, device=DEV), torch.ones(2, 1, 2, device=DEV))
    assert e.value.status == _lib.TAP_E_UNSUPPORTED
    torch.cuda.synchronize()


def _instances(B, n, seed):
    static, dynamic = synth.rand_instances(B, n, 2, seed=seed)
    tape = synth.random_feasible_tape(static, dynamic, n, seed=seed + 1)
    return static.to(DEV), dynamic.to(DEV), tape.to(DEV)


def test_episode_scores_net_through_the_pick():
    B, n, W, H = 33, 6, 5, 60
    static, _, tape = _instances(B, n, 21)
    net = DM.seeded(W, True, device=DEV, fused=True)
    plain = DM.seeded(W, True, device=DEV)
    net64 = DM.seeded(W, True, device=DEV, dtype=torch.float64)
    seen = []
    hook = plain.register_forward_hook(lambda m, i, o: seen.append(net64(i[0].double(), i[1].double())))
    try:
        want = T.pack.episode_scores_net(static, tape, RT, [W, H], plain)
    finally:
        hook.remove()
    assert len(seen) == n
    _lib.variant_hits_reset(DEV)
    got = T.pack.episode_scores_net(static, tape, RT, [W, H], net)
    assert _hits() == {_key((W, True)): n}
    whole = np.stack([DM.margin(p) for p in seen], 1).min(1) >= DM.MARGIN  # envs no step of which fell under the margin
    assert int((~whole).sum()) <= DM.CAP * B
    for u, v in zip(want, got):
        assert np.array_equal(u.cpu().numpy()[whole], v.cpu().numpy()[whole])


def test_run_episode_graph_replay():
    B, n, W, H, t = 64, 6, 5, 60, 'diff'
    static, dynamic, tape = _instances(B, n, 23)
    net = DM.seeded(W, True, device=DEV, fused=True)
    keys = ('tour_idx', 'place_x', 'pack_logp')
    with torch.no_grad():
        _lib.variant_hits_reset(DEV)
        out = T.run_episode(static, dynamic, T.TapePolicy(tape), W, H, reward_type=RT, heightmap_type=t, pack_policy=net)
        assert _hits() == {_key((W, True)): n}
        eager = {k: out[k].clone() for k in keys}
        env = T.BatchedContainer(B, [W, H], n, RT, t, device=DEV, place_at='container')
        prev = T.pack._binary_mode
        T.pack.set_binary_check('trust')
        try:
            s = torch.cuda.Stream(DEV)
            s.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(s):
                T.run_episode(static, dynamic, T.TapePolicy(tape), W, H, reward_type=RT, heightmap_type=t, pack_policy=net, env=env)
            torch.cuda.current_stream(DEV).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                gout = T.run_episode(static, dynamic, T.TapePolicy(tape), W, H, reward_type=RT, heightmap_type=t, pack_policy=net,
                                     env=env)
            for _ in range(2):
                g.replay()
                torch.cuda.synchronize()
                for k in keys:
                    assert torch.equal(gout[k], eager[k]), k
        finally:
            T.pack.set_binary_check(prev)
    assert tuple(eager['pack_logp'].shape) == (B, n)
