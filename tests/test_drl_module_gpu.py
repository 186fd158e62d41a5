"""tools.DRL on the MI355X.

Against the reference: the four actor fixtures (tests/golden/actor_*.npz, model.DRL.forward), the whole state dict loaded
strictly into ONE module on cuda:0, eval(), teacher-forced on the recorded tour through the head's GIVEN launch, grad enabled,
one backward() of the fixture's adv-weighted sum: tour_logp and every parameter's gradient under pointer_model.tolerance with
the fixture's own e_ref -- the rule of tests/test_actor_reference_gpu.py, whose tour_logp was float64 torch ops where the
module's is the head's fp32.

Against the recipe: the module issues the hand-wired recipe's launches, so free-running it returns the
recipe's bytes -- greedy in eval(), and in train() at p = 0.1 the bytes and gradients of the recipe driven by a StepDropout of
the same seed and PointerHeadPolicy.from_source.  And the whole forward replays from one graph, drawing anew each time."""
import numpy as np
import pytest
import torch

import actor_reference_cases as AC
import pointer_model as PM
import tap_net_amd as T
from tap_net_amd import _lib, pack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GIVEN = 3                                                       # the head's launch-record variant
SEED = 2024


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _actor(D, z, dropout=0., **kw):
    """the reference's arguments for the fixtures' actor; its whole state dict, strictly"""
    actor = T.DRL(D, 3 * AC.N, AC.HE, AC.HD, True, 'bot', True, 5, 50, D, "C+P+S-lb-soft", 'shape_heightmap', "diff", "LB_GREEDY",
                  pack.update_dynamic, pack.update_mask, 1, dropout, **kw)
    actor.load_state_dict(AC.state_dict(z), strict=True)
    return actor.to(DEV)


def _inputs(D):
    st, dy = AC.instances(D)
    B = AC.BATCH[D]
    zeros = (torch.zeros(B, D, 1, device=DEV), torch.zeros((B, 4, 1) if D == 2 else (B, 2, 5, 5), device=DEV))   # trainer.py:116-119
    return _dev(st), _dev(dy), zeros


def _hits():
    return {(kind, extra): sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == kind and k[5] == extra)
            for kind in (_lib.TAP_HIT_DECODER, _lib.TAP_HIT_HEIGHTMAP, _lib.TAP_HIT_POINTER, _lib.TAP_HIT_POLICY_PICK) for extra in (0, 1)}


_RUNS = {}


@pytest.fixture(params=AC.CASES, ids=["%dd-%s" % c for c in AC.CASES])
def run(request):
    """the module's teacher-forced episode and backward for one fixture, made once and left unchanged"""
    if request.param not in _RUNS:
        D, ws = request.param
        z = AC.load(D, ws)
        actor = _actor(D, z).eval()
        static, dynamic, zeros = _inputs(D)
        _lib.variant_hits_reset(DEV)
        with torch.enable_grad():
            tour_idx, tour_logp, none, reward = actor(static, dynamic, zeros, tour=_dev(z["tour_idx"].astype(np.int64)))
            assert none is None and tour_logp.dtype is torch.float32 and tour_logp.requires_grad
            (_dev(z["adv"]) * tour_logp.sum(1)).sum().backward()
        torch.cuda.synchronize()
        hits = _hits()
        given = sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == _lib.TAP_HIT_POLICY_PICK and k[3] == GIVEN and k[5] == 0)
        actor.last_stepper.check()
        cpu = lambda t: t.detach().cpu().numpy()                                                                 # noqa: E731
        _RUNS[request.param] = dict(z=z, D=D, ws=ws, hits=hits, given=given, tour=cpu(tour_idx), tour_logp=cpu(tour_logp).astype(np.float64),
                                    reward=cpu(reward), grads={k: cpu(p.grad).astype(np.float64) for k, p in actor.named_parameters()})
    return _RUNS[request.param]


def _held(label, rows):
    """rows of (name, got, want, e_ref): each within pointer_model.tolerance(e_ref, want); prints every figure first"""
    failed, worst = [], ("", 0.0)
    for name, got, want, e in rows:
        assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all(), name
        e, err = float(e), float(np.abs(got - want).max())
        tol = PM.tolerance(e, want)
        print("%s %s: err %.3g e_ref %.3g ratio %.2f tolerance %.3g max|want| %.3g" % (label, name, err, e, AC.ratio(err, e), tol,
                                                                                      np.abs(want).max()))
        if not (np.abs(want).max() > 0 and err <= tol):
            failed.append((name, err, tol))
        if AC.ratio(err, e) > worst[1]:
            worst = (name, AC.ratio(err, e))
    print("%s: worst err / e_ref %.2f (%s)" % (label, worst[1], worst[0]))
    assert not failed, (label, failed)


def test_module_gives_the_references_tour_logp_and_reward(run):
    z = run["z"]
    assert np.array_equal(run["tour"], z["tour_idx"])
    _held("DRL %dD %s" % (run["D"], run["ws"]), [("tour_logp", run["tour_logp"], z["tour_logp"], z["e_ref_tour_logp"])])
    err = float(np.abs(run["reward"].astype(np.float64) - z["neg_scores"].astype(np.float64)).max())
    print("DRL %dD %s reward: err %.3g" % (run["D"], run["ws"], err))
    assert run["reward"].shape == z["neg_scores"].shape and err <= 1e-6


def test_module_gives_the_references_gradients(run):
    z = run["z"]
    keys = sorted(k[len("sd_"):] for k in z if k.startswith("sd_"))
    assert len(keys) == AC.N_KEYS[run["D"]] and sorted(run["grads"]) == keys
    _held("DRL %dD %s gradient" % (run["D"], run["ws"]), [(k, run["grads"][k], z["grad_" + k], z["e_ref_grad_" + k]) for k in keys])


def test_the_modules_kernels_ran(run):
    """n launches of this dimension's decoder step and none of the other kind, n of the pointer, n of the head's GIVEN form and
    no other head form, and the same counts backward"""
    n, hits = AC.N, run["hits"]
    mine, other = (_lib.TAP_HIT_DECODER, _lib.TAP_HIT_HEIGHTMAP) if run["D"] == 2 else (_lib.TAP_HIT_HEIGHTMAP, _lib.TAP_HIT_DECODER)
    assert hits[(mine, 0)] == n and hits[(other, 0)] == 0, hits
    assert hits[(_lib.TAP_HIT_DECODER, 1)] == n and hits[(_lib.TAP_HIT_HEIGHTMAP, 1)] == 0, hits
    assert hits[(_lib.TAP_HIT_POINTER, 0)] == n and hits[(_lib.TAP_HIT_POINTER, 1)] == n, hits
    assert run["given"] == n and hits[(_lib.TAP_HIT_POLICY_PICK, 0)] == n and hits[(_lib.TAP_HIT_POLICY_PICK, 1)] == n, hits


class _Watch(object):
    """a ``stepper=`` that hands a real EpisodeStepper through and keeps the mask each pick was made under"""

    def __init__(self, sp):
        self._sp, self.seen = sp, []

    def __getattr__(self, name):
        return getattr(self._sp, name)

    def begin(self, static, dynamic):
        self.seen = []
        return self._sp.begin(static, dynamic)

    def step(self, ptr):
        self.seen.append(bool((self._sp.current_mask.gather(1, ptr.unsqueeze(1)) != 0).all()))
        return self._sp.step(ptr)


def _recipe(actor, static, dynamic, sd):
    """INTEGRATION 2i / 2m by hand on ``actor``'s children: -> tour_idx, tour_logp, reward.  ``sd``: the StepDropout of a
    training episode, None for the greedy one"""
    B, n, D = int(static.shape[0]), AC.N, actor.block_dim
    env = T.BatchedContainer(B, AC.CONTAINER[D], n, "C+P+S-lb-soft", "diff", device=DEV)
    sp = T.EpisodeStepper(static, dynamic, env, steps=n, expand_dynamic=False)
    pointer, state = actor.pointer, {"hh": None}
    if sd is not None:
        sd.next_episode()
    sf = pointer.fold_static(actor.static_encoder, static[:, 1:, :])
    fold = pointer.fold_episode(actor.dynamic_encoder, *pointer.fold_decoder(actor.static_decoder, actor.dynamic_decoder, combine='cat'))

    def scorer(step, decoder_static, decoder_dynamic, **_):
        if sd is None:
            logits, state["hh"] = pointer.forward_step(sf, sp.dynamic_bits, fold, decoder_static, decoder_dynamic, state["hh"])
        else:
            logits, state["hh"] = pointer.forward_step_dropout(sf, sp.dynamic_bits, fold, decoder_static, decoder_dynamic, state["hh"], sd)
        return logits
    pol = T.PointerHeadPolicy(scorer, greedy=True) if sd is None else T.PointerHeadPolicy.from_source(scorer, sd)
    out = T.run_episode(static, dynamic, pol, 5, 50, stepper=sp)
    return out["tour_idx"], pol.tour_logp(), out["reward"]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype is torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype is torch.float32 else b)


@pytest.mark.parametrize("D", [2, 3])
def test_free_running_module_is_the_recipe(D):
    """eval(): the greedy recipe's tour, tour_logp and reward bytes.  train() at p = 0.1: those of the recipe on a StepDropout
    of the same seed with PointerHeadPolicy.from_source, over two episodes, and every parameter's gradient; every pick is
    selectable under the mask of its step; the two training episodes differ"""
    z = AC.load(D, "sharp")
    static, dynamic, zeros = _inputs(D)
    actor, twin = _actor(D, z, 0.1, seed=SEED), _actor(D, z, 0.1)
    adv = _dev(z["adv"])
    with torch.no_grad():
        got, want = actor.eval()(static, dynamic, zeros), _recipe(twin.eval(), static, dynamic, None)
        for a, b in zip((got[0], got[1], got[3]), want):
            assert _same(a, b)
        assert bool(torch.isfinite(got[1]).all())
    actor.train(), twin.train()
    sd = T.StepDropout(SEED, DEV)
    watch = _Watch(T.EpisodeStepper(static, dynamic, T.BatchedContainer(AC.BATCH[D], AC.CONTAINER[D], AC.N, "C+P+S-lb-soft", "diff", device=DEV),
                                    steps=AC.N, expand_dynamic=False))
    tours = []
    for episode in (1, 2):
        with torch.enable_grad():
            got = actor(static, dynamic, zeros, stepper=watch if episode == 2 else None)
            tours.append(got[0].clone())
            (adv * got[1].sum(1)).sum().backward()
            want = _recipe(twin, static, dynamic, sd)
            (adv * want[1].sum(1)).sum().backward()
        for a, b in zip((got[0], got[1], got[3]), want):
            assert _same(a, b), episode
        assert actor.step_dropout(DEV).state.tolist() == [SEED, episode] == sd.state.tolist()
    assert watch.seen == [True] * AC.N and not torch.equal(tours[0], tours[1])
    for (k, p), (_, q) in zip(actor.named_parameters(), twin.named_parameters()):
        assert p.grad is not None and float(p.grad.abs().max()) > 0 and _same(p.grad, q.grad), k
    actor.last_stepper.check()


def test_forward_replays_from_one_graph():
    """actor(static, dynamic, decoder_input) captured once under no_grad in train() at the 2D fixture's shape: the episode
    counter advances inside the graph, so two replays give two tours, and replay k is, byte for byte, the k-th eager call
    (after the warm-up both modules make) of a second module with the same seed and weights"""
    z = AC.load(2, "sharp")
    static, dynamic, zeros = _inputs(2)
    actor, twin = _actor(2, z, 0.1, seed=SEED).train(), _actor(2, z, 0.1, seed=SEED).train()
    pack.set_binary_check('trust')
    try:
        with torch.no_grad():
            side = torch.cuda.Stream(device=DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                actor(static, dynamic, zeros)
            torch.cuda.current_stream(DEV).wait_stream(side)
            torch.cuda.synchronize()
            twin(static, dynamic, zeros)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                rec = actor(static, dynamic, zeros)
            torch.cuda.synchronize()
            assert actor.step_dropout(DEV).state.tolist() == [SEED, 1]       # captured, not run
            replays = []
            for k in (1, 2):
                graph.replay()
                torch.cuda.synchronize()
                assert actor.step_dropout(DEV).state.tolist() == [SEED, 1 + k]
                got = [rec[0].clone(), rec[1].clone(), rec[3].clone()]
                want = twin(static, dynamic, zeros)
                for a, b in zip(got, (want[0], want[1], want[3])):
                    assert _same(a, b), k
                assert bool(torch.isfinite(got[1]).all())
                replays.append(got)
            assert not torch.equal(replays[0][0], replays[1][0])
            actor.last_stepper.check()
            pack.check_binary()
    finally:
        pack.set_binary_check('check')
