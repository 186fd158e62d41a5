"""tap_net_amd.trainer without a GPU: the torch forms of the training tail in float64 -- the model the device path is tested
against (tests/test_train_tail_gpu.py) -- held to ``clip_grad_norm_`` + ``torch.optim.Adam`` and to the reference's three loss
lines, and ``TrainStep.step`` held to the reference's iteration (trainer.py:200-236) driven by stock torch."""
import copy
import re

import numpy as np
import pytest
import torch

import actor_reference_cases as AC
import pointer_model as PM
import tap_net_amd as T
import train_tail_model as TM
from tap_net_amd import _lib, trainer
from test_drl_module_cpu import RecordedStepper, reference_args

SHAPES = [(1,), (63,), (64, 3), (65,), (1, 1, 64), (130, 17)]


def _params(seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=dtype)) for s in SHAPES]


def _grads(params, step, seed):
    """gradients whose total norm alternates between about 500 (clipped) and about 0.5 (not)"""
    g = torch.Generator().manual_seed(1000 * seed + step)
    raw = [torch.randn(p.shape, generator=g, dtype=p.dtype) for p in params]
    norm = torch.sqrt(sum((r * r).sum() for r in raw))
    return [r * ((500.0 if step % 2 == 0 else 0.5) / norm) for r in raw]


def test_clip_adam_torch_path_is_clip_grad_norm_and_adam():
    """two groups with their own lr and max_norm, four steps, float64: every parameter within 1e-12 relative"""
    mine = [_params(1), _params(2)]
    theirs = [[torch.nn.Parameter(p.detach().clone()) for p in ps] for ps in mine]
    cfg = [(1e-3, 2.0), (5e-4, 1.0)]
    opt = T.ClipAdam([(ps, lr, mx) for ps, (lr, mx) in zip(mine, cfg)])
    assert not opt.on_device
    stock = [torch.optim.Adam(ps, lr=lr) for ps, (lr, _) in zip(theirs, cfg)]
    for step in range(4):
        norms = []
        for gi in range(2):
            for p, q, g in zip(mine[gi], theirs[gi], _grads(mine[gi], step, gi)):
                p.grad.add_(g)                                  # what autograd does: accumulate in place
                q.grad = g.clone()
            norms.append(float(torch.nn.utils.clip_grad_norm_(theirs[gi], cfg[gi][1])))
            stock[gi].step()
        opt.step()
        assert np.allclose(opt.grad_norm.numpy(), norms, rtol=1e-6) and (norms[0] > 100) == (step % 2 == 0)
        for gi in range(2):
            for p, q in zip(mine[gi], theirs[gi]):
                err = float((p - q).detach().abs().max() / q.detach().abs().max().clamp_min(1e-30))
                assert err <= 1e-12, (step, gi, tuple(p.shape), err)
                assert float(p.grad.abs().max()) == 0.0         # zeroed by the step
    assert opt.steps[:, 0].tolist() == [4, 4] and opt.skipped == 0


def test_a_tensor_without_gradient_keeps_its_bytes():
    ps = _params(3)
    opt = T.ClipAdam([(ps, 1e-2, 1.0)])
    before = [p.detach().clone() for p in ps]
    for step in range(2):
        for p, g in list(zip(ps, _grads(ps, step, 0)))[1:]:
            p.grad.add_(g)
        opt.step()
    assert torch.equal(ps[0].detach(), before[0])
    assert all(not torch.equal(p.detach(), b) for p, b in list(zip(ps, before))[1:])
    g, m, v = opt.views(ps[0])
    assert float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0 and g.data_ptr() == ps[0].grad.data_ptr()


def test_a_gradient_that_is_not_finite_skips_its_group_alone():
    a, b = _params(4), _params(5)
    opt = T.ClipAdam([(a, 1e-3, 1.0), (b, 1e-3, 1.0)])
    before = [p.detach().clone() for p in a + b]
    for p, g in zip(a, _grads(a, 0, 0)):
        p.grad.add_(g)
    a[3].grad.view(-1)[7] = float('inf')
    for p, g in zip(b, _grads(b, 0, 1)):
        p.grad.add_(g)
    opt.step()
    assert all(torch.equal(p.detach(), q) for p, q in zip(a, before[:len(a)]))
    assert all(not torch.equal(p.detach(), q) for p, q in zip(b, before[len(a):]))
    assert opt.skipped == 1 and opt.steps[:, 0].tolist() == [0, 1]
    assert all(float(p.grad.abs().max()) == 0.0 for p in a + b)
    assert all(float(t.abs().max()) == 0.0 for p in a for t in opt.views(p)[1:])


def test_state_dict_round_trips():
    a, b = _params(6), _params(6)
    one, two = T.ClipAdam([(a, 1e-3, 1.0)]), T.ClipAdam([(b, 7.0, 9.0)])
    for step in range(3):
        for p, g in zip(a, _grads(a, step, 0)):
            p.grad.add_(g)
        one.step()
    sd = copy.deepcopy(one.state_dict())
    two.load_state_dict(sd)
    with torch.no_grad():
        for p, q in zip(a, b):
            q.copy_(p)
    for opt, ps in ((one, a), (two, b)):
        for p, g in zip(ps, _grads(a, 3, 0)):
            p.grad.add_(g)
        opt.step()
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(a, b)) and two.steps[0, 0] == 4
    got = two.state_dict()
    assert set(got) == {"exp_avg", "exp_avg_sq", "steps", "skipped", "hyper"} and got["hyper"][0, 0] == 1e-3
    with pytest.raises(ValueError):
        T.ClipAdam([(a[:2], 1e-3, 1.0)]).load_state_dict(sd)


@pytest.mark.parametrize("flagged", ["none", "first", "last", "all"])
def test_reinforce_losses_torch_form_is_the_references_lines(flagged):
    """values and gradients; with flagged envs the reference's lines over the other envs, the divisor still B"""
    B, n = 7, 5
    g = torch.Generator().manual_seed(11)
    reward, est0, logp0 = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((B,), (B,), (B, n)))
    keep = {"none": slice(0, B), "first": slice(1, B), "last": slice(0, B - 1), "all": slice(0, 0)}[flagged]
    bad = torch.ones(B, dtype=torch.bool)
    bad[keep] = False
    reward[bad] = float('nan')
    est, logp = est0.clone().requires_grad_(), logp0.clone().requires_grad_()
    actor_loss, critic_loss = T.reinforce_losses(reward, est, logp)
    (3.0 * actor_loss + 0.5 * critic_loss).backward()
    est2, logp2 = est0.clone().requires_grad_(), logp0.clone().requires_grad_()
    k = int((~bad).sum())
    if k:
        a2, c2 = TM.reference_lines(reward[keep], est2[keep], logp2[keep])
        a2, c2 = a2 * k / B, c2 * k / B
        (3.0 * a2 + 0.5 * c2).backward()
        want_e, want_l = est2.grad, logp2.grad
    else:
        a2 = c2 = torch.zeros((), dtype=torch.float64)
        want_e, want_l = torch.zeros_like(est0), torch.zeros_like(logp0)
    assert abs(float((actor_loss - a2).detach())) <= 1e-14 and abs(float((critic_loss - c2).detach())) <= 1e-14
    assert float((est.grad - want_e).abs().max()) <= 1e-15 and float((logp.grad - want_l).abs().max()) <= 1e-15
    adv, seed_logp, seed_est, stats = T.reinforce_seeds(reward, est0, logp0)
    m = TM.losses_model(reward.numpy(), est0.numpy(), logp0.numpy())
    for got, want in zip((adv, seed_logp, seed_est, stats), m):
        assert got.shape == want.shape and np.abs(got.numpy() - want).max() <= 1e-14
    assert stats[4] == B - k and bool(torch.isfinite(stats).all())


def _drive_reference(actor, critic, optims, z, st, dyn, dec, tour, max_norm):
    """trainer.py:200-236 on stock torch"""
    critic_est = critic(st[:, 1:3, :], dyn).view(-1)
    _, tour_logp, _, reward = actor(st, dyn, dec, tour=tour, stepper=RecordedStepper(z, 2))
    actor_loss, critic_loss = TM.reference_lines(reward, critic_est, tour_logp)
    for optim, loss, module in ((optims[0], actor_loss, actor), (optims[1], critic_loss, critic)):
        optim.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(module.parameters(), max_norm)
        optim.step()
    return actor_loss, critic_loss


def test_train_step_is_the_references_iteration():
    """float64, the recorded stepper, ``tour=`` forced, two iterations: every parameter of both modules within 1e-10 of the
    same modules driven by the reference's lines, two backwards, two clip_grad_norm_ and two torch.optim.Adam"""
    z = AC.load(2, "init")
    actor = reference_args(2)
    actor.load_state_dict(AC.state_dict(z), strict=True)
    torch.manual_seed(3)
    critic = T.StateCritic(2, 3 * AC.N, 64)
    for p in critic.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    actor.double(), critic.double()
    actor2, critic2 = copy.deepcopy(actor), copy.deepcopy(critic)
    st, dyn = (torch.from_numpy(np.asarray(a, np.float64)) for a in AC.instances(2))
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))             # noqa: E731
    dec = [t(z["decoder_static"][0]), t(z["decoder_dynamic"][0])]
    tour = torch.from_numpy(z["tour_idx"].astype(np.int64))
    lrs, max_norm = (5e-3, 1e-2), 0.05
    ts = T.TrainStep(actor, critic, lrs[0], lrs[1], max_norm, 2, 'shape_heightmap')
    optims = [torch.optim.Adam(actor2.parameters(), lr=lrs[0]), torch.optim.Adam(critic2.parameters(), lr=lrs[1])]
    start = [p.detach().clone() for p in actor.parameters()]
    for it in range(2):
        stats = ts.step(st, dyn, dec[0], dec[1], tour=tour, stepper=RecordedStepper(z, 2))
        want = _drive_reference(actor2, critic2, optims, z, st, dyn, dec, tour, max_norm)
        assert abs(float(stats[0] - want[0].detach())) <= 1e-12 and abs(float(stats[1] - want[1].detach())) <= 1e-12 and stats[4] == 0
    assert float(ts.optim.grad_norm.min()) > max_norm                       # both groups were clipped
    moved = 0.0
    for m, m2 in ((actor, actor2), (critic, critic2)):
        for (k, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
            assert float((p - q).detach().abs().max()) <= 1e-10 * max(1.0, float(q.detach().abs().max())), k
    for p, q in zip(actor.parameters(), start):
        moved = max(moved, float((p.detach() - q).abs().max()))
    assert moved > 1e-3


def test_the_export_list_is_the_headers():
    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(tap_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in ("tap_reinforce_losses", "tap_reinforce_losses_scratch", "tap_clip_adam_norm", "tap_clip_adam_apply"):
        assert name in declared and hasattr(_lib.lib(), name)
    assert _lib.lib().tap_abi_version() == 1
    assert _lib.lib().tap_reinforce_losses_scratch(257) == 8 + 2 * 5 * 8
    for name in trainer.__all__:
        assert getattr(T, name) is getattr(trainer, name) and name in T.__all__


@pytest.mark.parametrize("strategy", ["pre_train", "none_train"])
def test_the_pack_net_strategies_raise(strategy):
    actor = reference_args(2)
    actor.packing_strategy = strategy
    with pytest.raises(NotImplementedError, match=strategy):
        T.TrainStep(actor, T.StateCritic(2, 3 * AC.N, 64), 1e-3, 1e-3, 2.0, 2, 'shape_heightmap')


@pytest.mark.parametrize("t", [0, 1, 999])
@pytest.mark.parametrize("chunk", [64, 256])
def test_torchs_float32_step_stays_inside_the_floor_on_the_gpu_cases(chunk, t):
    """the inputs of tests/test_train_tail_gpu.py's clip-and-Adam cases are ones on which the update is a smooth function of
    g: torch's own float32 step is within 16 ulp of the largest wanted value of the float64 model, for p, m and v"""
    for group in TM.tail_case(chunk, t, seed=5 + t):
        args = [group[k] for k in ("p", "g", "m", "v", "t", "lr", "max_norm")]
        want, got = TM.adam_model(*args), TM.adam_torch(*args)
        for name, ws, gs in zip("pmv", want[:3], got[:3]):
            w, g = np.concatenate(ws), np.concatenate(gs)
            e_ref = float(np.abs(w - g).max())
            assert e_ref <= 16.0 * PM.U32 * float(np.abs(w).max()), (t, name, e_ref)
        assert abs(want[3] - got[3]) <= 16.0 * PM.U32 * want[3]
