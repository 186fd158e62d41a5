"""tap_net_amd.trainer on the MI355X at the actor fixture's 2D shape (He = 32, Hd = 64, tests/golden/actor_2d_init.npz's
weights) with a StateCritic of H = 64: TrainStep.step against the hand-composed recipe (bytes) and against stock torch's tail
on the same gradients (pointer_model.tolerance), the whole iteration replayed from one graph, and train() / validate() end to
end on a data set of eight instances."""
import os

import numpy as np
import pytest
import torch

import actor_reference_cases as AC
import golden_util as G
import pointer_model as PM
import tap_net_amd as T
import train_tail_model as TM
from tap_net_amd import pack, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 77
LRS, MAX_NORM = (5e-4, 5e-4), 2.0                               # the reference's defaults


def _modules(dropout=0.):
    z = AC.load(2, "init")
    actor = T.DRL(2, 3 * AC.N, AC.HE, AC.HD, True, 'bot', True, 5, 50, 2, "C+P+S-lb-soft", 'shape_heightmap', "diff", "LB_GREEDY",
                  pack.update_dynamic, pack.update_mask, 1, dropout, seed=SEED)
    actor.load_state_dict(AC.state_dict(z), strict=True)
    torch.manual_seed(3)
    critic = T.StateCritic(2, 3 * AC.N, 64)
    for p in critic.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    return actor.to(DEV).train(), critic.to(DEV).train()


_DATA = {}


def _batch(B, start=0):
    """B instances of the committed 2D data set from ``start`` on, the trainer's zero decoder inputs, a feasible tour"""
    if (B, start) not in _DATA:
        ds = G.load("dataset_2d.npz")
        idx = (np.arange(B) + start) % ds["static"].shape[0]
        st, dy = ds["static"][idx].astype(np.float32), ds["dynamic"][idx].astype(np.float32)
        tour = synth.random_feasible_tape(st, dy, AC.N, seed=1 + start)
        _DATA[(B, start)] = ([torch.from_numpy(st).to(DEV), torch.from_numpy(dy).to(DEV), torch.zeros(B, 2, 1, device=DEV),
                              torch.zeros(B, 4, 1, device=DEV)], torch.as_tensor(tour).to(DEV))
    return _DATA[(B, start)]


def _bytes(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _params(*modules):
    return [(k, p) for m in modules for k, p in m.named_parameters()]


def _recipe_step(actor, critic, optim, batch, tour):
    """TrainStep.step's calls one by one"""
    static, dynamic, decoder_static, decoder_dynamic = batch
    critic_est = critic(static[:, 1:3, :], pack.dynamic_bits(dynamic)[0]).view(-1)
    _, tour_logp, _, reward = actor(static, dynamic, [decoder_static, decoder_dynamic], tour=tour)
    _, seed_logp, seed_est, stats = T.reinforce_seeds(reward, critic_est, tour_logp)
    torch.autograd.backward([tour_logp, critic_est], [seed_logp, seed_est])
    optim.step()
    return stats


@pytest.mark.parametrize("B", [6, 130])
def test_train_step_is_the_hand_composed_recipe(B):
    """two iterations: the parameter bytes and the stats rows of the same calls made one by one"""
    batch, tour = _batch(B)
    actor, critic = _modules()
    actor2, critic2 = _modules()
    ts = T.TrainStep(actor, critic, LRS[0], LRS[1], MAX_NORM, 2, 'shape_heightmap', tail='hip')
    optim = T.ClipAdam([(list(actor2.parameters()), LRS[0], MAX_NORM), (list(critic2.parameters()), LRS[1], MAX_NORM)])
    start = [_bytes(p) for _, p in _params(actor, critic)]
    for it in range(2):
        got, want = ts.step(*batch, tour=tour), _recipe_step(actor2, critic2, optim, batch, tour)
        assert _bytes(got) == _bytes(want) and bool(torch.isfinite(got).all()) and float(got[4]) == 0
    for (k, p), (_, q) in zip(_params(actor, critic), _params(actor2, critic2)):
        assert _bytes(p) == _bytes(q), k
    assert sum(a != _bytes(p) for a, (_, p) in zip(start, _params(actor, critic))) >= 24      # every tensor but the few whose input is zero moved
    assert ts.optim.steps[:, 0].tolist() == [2, 2] and ts.optim.skipped == 0
    actor.last_stepper.check()


@pytest.mark.parametrize("B", [6, 130])
def test_one_iteration_from_warm_moments_against_stock_torch(B):
    """the gradients of one iteration; then this package's two launches against the float64 model of clip_grad_norm_ + Adam on
    those gradients, e_ref being stock torch's float32 step on them"""
    batch, tour = _batch(B)
    actor, critic = _modules()
    ts = T.TrainStep(actor, critic, LRS[0], LRS[1], MAX_NORM, 2, 'shape_heightmap', tail='hip')
    rng = np.random.RandomState(B)
    with torch.no_grad():
        for m in (actor, critic):
            for p in m.parameters():
                _, mm, vv = ts.optim.views(p)
                mm.copy_(torch.from_numpy(rng.uniform(-1e-2, 1e-2, tuple(p.shape)).astype(np.float32)))
                vv.copy_(torch.from_numpy(rng.uniform(1e-4, 1.0, tuple(p.shape)).astype(np.float32)))
    sd = ts.optim.state_dict()
    sd["steps"][:] = 100
    ts.optim.load_state_dict(sd)
    tour_logp, critic_est, reward = ts.forward(*batch, tour=tour)
    _, seed_logp, seed_est, _ = T.reinforce_seeds(reward, critic_est, tour_logp)
    torch.autograd.backward([tour_logp, critic_est], [seed_logp, seed_est])
    cpu = lambda t: t.detach().cpu().numpy().copy()                        # noqa: E731
    before = [[(cpu(p),) + tuple(cpu(t) for t in ts.optim.views(p)) for p in m.parameters()] for m in (actor, critic)]
    ts.optim.step()
    torch.cuda.synchronize()
    for gi, (m, rows) in enumerate(zip((actor, critic), before)):
        p, g, mm, vv = ([r[i] for r in rows] for i in range(4))
        assert max(float(np.abs(x).max()) for x in g) > 0
        want, ref = TM.adam_model(p, g, mm, vv, 100, LRS[gi], MAX_NORM), TM.adam_torch(p, g, mm, vv, 100, LRS[gi], MAX_NORM)
        got = ([cpu(q) for q in m.parameters()], [cpu(ts.optim.views(q)[1]) for q in m.parameters()], [cpu(ts.optim.views(q)[2]) for q in m.parameters()])
        cat = lambda xs: np.concatenate([np.asarray(x, np.float64).ravel() for x in xs])    # noqa: E731
        for name, a, w, r in zip(("p", "exp_avg", "exp_avg_sq"), got, want[:3], ref[:3]):
            a, w, r = cat(a), cat(w), cat(r)
            err, tol = float(np.abs(a - w).max()), PM.tolerance(float(np.abs(r - w).max()), w)
            print("warm B %d group %d %s: err %.3g tolerance %.3g" % (B, gi, name, err, tol))
            assert err <= tol, (gi, name, err, tol)
        assert abs(float(ts.optim.grad_norm[gi]) - want[3]) <= PM.tolerance(abs(ref[3] - want[3]), np.array([want[3]]))


@pytest.mark.parametrize("B", [6, 130])
def test_the_iteration_replays_from_one_graph(B):
    """train() mode at dropout 0.1, no tour: capture, then two replays on two different batches, are byte for byte two eager
    iterations of a twin with the same seed and episode counter -- stats rows and every parameter"""
    actor, critic = _modules(0.1)
    actor2, critic2 = _modules(0.1)
    ts = T.TrainStep(actor, critic, LRS[0], LRS[1], MAX_NORM, 2, 'shape_heightmap', tail='hip')
    twin = T.TrainStep(actor2, critic2, LRS[0], LRS[1], MAX_NORM, 2, 'shape_heightmap', tail='hip')
    pack.set_binary_check('trust')
    try:
        ts.capture(*_batch(B)[0])
        torch.cuda.synchronize()
        assert actor.step_dropout(DEV).state.tolist() == [SEED, 0] and ts.optim.steps[:, 0].tolist() == [0, 0]
        for (k, p), (_, q) in zip(_params(actor, critic), _params(actor2, critic2)):
            assert _bytes(p) == _bytes(q), k                                # the warm-up was undone
        rows = []
        for it, start in enumerate((0, B)):
            batch = _batch(B, start)[0]
            got = ts.replay(*batch).clone()
            want = twin.step(*batch)
            torch.cuda.synchronize()
            assert _bytes(got) == _bytes(want) and bool(torch.isfinite(got).all()), it
            assert actor.step_dropout(DEV).state.tolist() == [SEED, it + 1] == actor2.step_dropout(DEV).state.tolist()
            for (k, p), (_, q) in zip(_params(actor, critic), _params(actor2, critic2)):
                assert _bytes(p) == _bytes(q), (it, k)
            rows.append(_bytes(got))
        assert rows[0] != rows[1] and ts.optim.steps[:, 0].tolist() == [2, 2]
        actor.last_stepper.check()
        pack.check_binary()
    finally:
        pack.set_binary_check('check')


def test_train_end_to_end(tmp_path, monkeypatch, capsys):
    """eight instances from pack.create_dataset (10 blocks, W = 5), batch 4, one epoch, everything under tmp_path"""
    monkeypatch.chdir(tmp_path)
    tr, va = pack.create_dataset(10, 8, 8, 2, 7, 50, 1, [1, 5], seed=5, device=DEV)
    train_data = T.PACKDataset(tr, 10, 8, 1, "bot", "diff", True, 5, unit=1)
    valid_data = T.PACKDataset(va, 10, 8, 2, "bot", "diff", True, 5, unit=1)
    actor, critic = _modules(0.1)
    start = [_bytes(p) for _, p in _params(actor, critic)]
    kwargs = dict(num_nodes=10, obj_dim=2, input_type='bot', reward_type='C+P+S-lb-soft', packing_strategy='LB_GREEDY', container_width=5,
                  note='t', actor_lr=5e-4, critic_lr=5e-4, max_grad_norm=2.0, train_data=train_data, valid_data=valid_data, batch_size=4,
                  train_size=8, valid_size=8, epoch_num=1, task='train', use_cuda=True, decoder_input_type='shape_heightmap', render_fn=None)
    save_dir = T.train(actor, critic, **kwargs)
    out = capsys.readouterr().out
    assert '    Epoch 0  Batch 1/2, reward: ' in out and 'Epoch 0,  mean epoch reward: ' in out
    assert save_dir.startswith(os.path.join('pack', '10', '2d-bot-C+P+S-lb-soft-LB_GREEDY-width-5-note-t-'))
    fresh_actor, fresh_critic = _modules(0.1)
    for where in (os.path.join(save_dir, 'checkpoints', '0'), save_dir):
        fresh_actor.load_state_dict(torch.load(os.path.join(where, 'actor.pt'), map_location=DEV), strict=True)
        fresh_critic.load_state_dict(torch.load(os.path.join(where, 'critic.pt'), map_location=DEV), strict=True)
    for (k, p), (_, q) in zip(_params(actor, critic), _params(fresh_actor, fresh_critic)):
        assert _bytes(p) == _bytes(q), k
    losses, rewards = np.loadtxt(os.path.join(save_dir, 'losses.txt'), ndmin=1), np.loadtxt(os.path.join(save_dir, 'reawrds.txt'), ndmin=1)
    assert losses.shape == (1,) and rewards.shape == (1,) and np.isfinite(losses).all() and np.isfinite(rewards).all()
    assert os.path.isdir(os.path.join(save_dir, 'render', '0'))
    assert sum(a != _bytes(p) for a, (_, p) in zip(start, _params(actor, critic))) >= 24
    mean = T.validate(torch.utils.data.DataLoader(valid_data, 8), actor, str(tmp_path / 'v'), **kwargs)
    assert np.isfinite(mean) and mean < 0 and actor.training
