"""The three launches of csrc/train.hip on the MI355X against the float64 model (tests/train_tail_model.py) under the
project's rule, pointer_model.tolerance: 4 e_ref + 16 ulp of the largest wanted value, e_ref being the error of torch's own
float32 form of the same arithmetic (the loss lines; ``clip_grad_norm_`` + non-fused ``Adam``) against the model."""
import numpy as np
import pytest
import torch

import pointer_model as PM
import tap_net_amd as T
import train_tail_model as TM
from tap_net_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = -12345.5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bytes(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _held(label, rows):
    failed = []
    for name, got, want, ref in rows:
        got, want, ref = (np.asarray(a, np.float64) for a in (got, want, ref))
        assert got.shape == want.shape and np.isfinite(got).all(), (label, name)
        e_ref, err = float(np.abs(ref - want).max()), float(np.abs(got - want).max())
        tol = PM.tolerance(e_ref, want) if want.size else 0.0
        print("%s %s: err %.3g e_ref %.3g tolerance %.3g max|want| %.3g" % (label, name, err, e_ref, tol, np.abs(want).max()))
        if err > tol:
            failed.append((name, err, tol))
    assert not failed, (label, failed)


# ---- the losses ---------------------------------------------------------------------------------------------------------
def _losses_launch(reward, est, logp, pad=64):
    """tap_reinforce_losses on buffers with ``pad`` canary floats behind every output -> the four buffers"""
    B, n = (int(v) for v in logp.shape)
    outs = [torch.full((k + pad,), CANARY, dtype=torch.float32, device=DEV) for k in (B, B * n, B, 5)]
    need = int(_lib.lib().tap_reinforce_losses_scratch(B))
    scratch = torch.zeros(need // 8, dtype=torch.int64, device=DEV)
    c = _lib.ctx(torch.device(DEV))
    for _ in range(2):                                          # the second launch finds the ticket the first one put back
        _lib.check(_lib.lib().tap_reinforce_losses(c, _lib.ptr(reward), _lib.ptr(est), _lib.ptr(logp), B, n, *[_lib.ptr(o) for o in outs],
                                                   _lib.ptr(scratch), need, _lib.stream_of(torch.device(DEV))), c)
    torch.cuda.synchronize()
    assert int(scratch[0]) == 0
    return outs, (B, B * n, B, 5)


def _losses_float32(reward, est, logp):
    """torch's float32 form: the reference's lines over the envs with a finite reward, the divisor B"""
    B, n = logp.shape
    ok = torch.isfinite(reward)
    k = int(ok.sum())
    adv = torch.where(ok, reward - est, torch.zeros_like(reward))
    stats = torch.zeros(5)
    if k:
        a, c = TM.reference_lines(reward[ok], est[ok], logp[ok])
        stats[:4] = torch.stack([a * k / B, c * k / B, reward[ok].mean() * k / B, est[ok].mean() * k / B])
    stats[4] = B - k
    return adv.numpy(), (adv / B).unsqueeze(1).expand(B, n).numpy(), (-2 * adv / B).numpy(), stats.numpy()


@pytest.mark.parametrize("n", [1, 10])
@pytest.mark.parametrize("B", [1, 3, 64, 65, 130, 1025])
def test_reinforce_losses_against_the_model(B, n):
    """values and seeds within the rule, canaries intact, the same bytes on two calls; no flagged env, the first, the last, all"""
    rng = np.random.RandomState(100 * B + n)
    for flagged in ("none", "first", "last", "all"):
        reward = -rng.uniform(0.2, 1.0, B).astype(np.float32)
        est = (reward + rng.normal(0, 0.2, B)).astype(np.float32)
        logp = -rng.uniform(0.01, 2.5, (B, n)).astype(np.float32)
        bad = {"none": [], "first": [0], "last": [B - 1], "all": list(range(B))}[flagged]
        reward[bad] = np.nan
        want = TM.losses_model(reward, est, logp)
        ref = _losses_float32(*(torch.from_numpy(a) for a in (reward, est, logp)))
        r, e, lp = _dev(reward), _dev(est), _dev(logp)
        outs, sizes = _losses_launch(r, e, lp)
        for o, k in zip(outs, sizes):
            assert bool((o[k:] == CANARY).all())
        got = [o[:k].cpu().numpy() for o, k in zip(outs, sizes)]
        got[1] = got[1].reshape(B, n)
        _held("losses B %d n %d %s" % (B, n, flagged), [(nm, g, w, rf) for nm, g, w, rf in zip(("adv", "seed_logp", "seed_est", "stats"), got, want, ref)])
        assert got[3][4] == len(bad)
        if bad:
            assert (got[0][bad] == 0).all() and (got[1][bad] == 0).all() and (got[2][bad] == 0).all()
        again = T.reinforce_seeds(r, e, lp)                          # the public call: the same bytes
        for o, k, a in zip(outs, sizes, again):
            assert _bytes(o[:k]) == _bytes(a)


def test_reinforce_losses_backward_on_the_device():
    B, n = 130, 10
    rng = np.random.RandomState(9)
    reward, est, logp = _dev(-rng.uniform(0.2, 1, B).astype(np.float32)), _dev(rng.normal(-0.5, 0.2, B).astype(np.float32)), \
        _dev(-rng.uniform(0.01, 2.5, (B, n)).astype(np.float32))
    est.requires_grad_(), logp.requires_grad_()
    a, c = T.reinforce_losses(reward, est, logp)
    (2.0 * a + 3.0 * c).backward()
    _, seed_logp, seed_est, stats = T.reinforce_seeds(reward, est, logp)
    assert _bytes(a) == _bytes(stats[0]) and _bytes(c) == _bytes(stats[1])
    assert torch.equal(logp.grad, 2.0 * seed_logp) and torch.equal(est.grad, 3.0 * seed_est)


# ---- clip + Adam ----------------------------------------------------------------------------------------------------------
def _make(chunk, t, seed, zero_grads=True):
    """the case's two groups as parameters on the device -- group 0's second tensor a view at element offset 1, and one extra
    tensor of 300 elements with a zero gradient and zero moments at the end of group 0 -- in a ClipAdam with the case's
    moments and counters loaded -> (optimizer, the groups' parameters, the case)"""
    case = TM.tail_case(chunk, t, seed)
    params = []
    for gi, group in enumerate(case):
        ps = []
        for i, p in enumerate(group["p"]):
            if gi == 0 and i == 1:
                base = torch.zeros(p.size + 1, dtype=torch.float32, device=DEV)
                base[1:] = _dev(p)
                ps.append(torch.nn.Parameter(base[1:]))
                assert ps[-1].data_ptr() % 16 == 4
            else:
                ps.append(torch.nn.Parameter(_dev(p)))
        if gi == 0:
            ps.append(torch.nn.Parameter(torch.linspace(-1, 1, 300, device=DEV)))
        params.append(ps)
    opt = T.ClipAdam([(ps, g["lr"], g["max_norm"]) for ps, g in zip(params, case)], chunk=chunk, zero_grads=zero_grads)
    assert opt.on_device
    for ps, group in zip(params, case):
        for p, g, m, v in zip(ps, group["g"], group["m"], group["v"]):
            gv, mv, vv = opt.views(p)
            gv.copy_(_dev(g)), mv.copy_(_dev(m)), vv.copy_(_dev(v))
            assert gv.data_ptr() % 16 == 0 and p.grad.data_ptr() == gv.data_ptr()
    sd = opt.state_dict()
    sd["steps"][:] = t
    opt.load_state_dict(sd)
    return opt, params, case


@pytest.mark.parametrize("t", [0, 1, 999])
@pytest.mark.parametrize("chunk", [64, 256])
def test_clip_adam_against_the_model(chunk, t):
    opt, params, case = _make(chunk, t, seed=5 + t)
    twin, tparams, _ = _make(chunk, t, seed=5 + t)
    assert int(opt._ranges[1, 1]) > (1024 if chunk == 64 else 256)                          # more partials than one LDS tile holds
    still = _bytes(params[0][-1])
    opt.step(), twin.step()
    torch.cuda.synchronize()
    cat = lambda xs: np.concatenate([np.asarray(x, np.float64).ravel() for x in xs])        # noqa: E731
    for gi, group in enumerate(case):
        args = [group[k] for k in ("p", "g", "m", "v", "t", "lr", "max_norm")]
        want, ref = TM.adam_model(*args), TM.adam_torch(*args)
        ps = params[gi][:len(group["p"])]
        got = ([p.detach().cpu().numpy() for p in ps], [opt.views(p)[1].cpu().numpy() for p in ps], [opt.views(p)[2].cpu().numpy() for p in ps])
        _held("clip adam chunk %d t %d group %d" % (chunk, t, gi),
              [(nm, cat(g), cat(w), cat(r)) for nm, g, w, r in zip(("p", "exp_avg", "exp_avg_sq"), got, want[:3], ref[:3])] +
              [("norm", [float(opt.grad_norm[gi])], [want[3]], [ref[3]])])
        assert (want[3] > group["max_norm"]) == (gi == 0)                                   # group 0 clipped, group 1 not
        assert float(np.abs(cat(want[0]) - cat(group["p"])).max()) > 1e-5                   # the step moved something
    assert opt.steps[:, 0].tolist() == [t + 1, t + 1] and opt.skipped == 0
    assert _bytes(params[0][-1]) == still                                                   # the zero-gradient tensor
    for ps, qs in zip(params, tparams):
        for p, q in zip(ps, qs):
            assert float(p.grad.abs().max()) == 0.0
            assert _bytes(p) == _bytes(q) and all(_bytes(a) == _bytes(b) for a, b in zip(opt.views(p), twin.views(q)))


def test_zero_grads_false_leaves_the_gradients():
    opt, params, case = _make(64, 1, seed=3, zero_grads=False)
    before = [_bytes(p.grad) for ps in params for p in ps]
    opt.step()
    torch.cuda.synchronize()
    assert before == [_bytes(p.grad) for ps in params for p in ps] and opt.steps[:, 0].tolist() == [2, 2]
    opt.zero_grad()
    assert all(float(p.grad.abs().max()) == 0.0 for ps in params for p in ps)


def test_an_inf_in_one_groups_gradient_skips_that_group_alone():
    opt, params, case = _make(64, 1, seed=4)
    twin, tparams, _ = _make(64, 1, seed=4)
    params[0][4].grad[3] = float('inf')
    before = [[_bytes(p)] + [_bytes(t) for t in opt.views(p)[1:]] for p in params[0]]
    opt.step(), twin.step()
    torch.cuda.synchronize()
    assert before == [[_bytes(p)] + [_bytes(t) for t in opt.views(p)[1:]] for p in params[0]]
    assert all(float(p.grad.abs().max()) == 0.0 for ps in params for p in ps)
    assert opt.skipped == 1 and opt.steps[:, 0].tolist() == [1, 2] and not np.isfinite(float(opt.grad_norm[0]))
    for p, q in zip(params[1], tparams[1]):                                                 # the other group stepped as ever
        assert _bytes(p) == _bytes(q)


def test_both_launches_replay_from_a_graph():
    """captured once, replayed three times: the bytes of three eager steps, and the counter reads 3"""
    eager, eparams, _ = _make(256, 0, seed=6, zero_grads=False)
    opt, params, _ = _make(256, 0, seed=6, zero_grads=False)
    for _ in range(3):
        eager.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert opt.steps[:, 0].tolist() == [0, 0]                                               # captured, not run
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert opt.steps[:, 0].tolist() == [3, 3] == eager.steps[:, 0].tolist()
    for ps, qs in zip(params, eparams):
        for p, q in zip(ps, qs):
            assert _bytes(p) == _bytes(q) and all(_bytes(a) == _bytes(b) for a, b in zip(opt.views(p), eager.views(q)))
