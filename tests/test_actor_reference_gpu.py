"""The reference's own actor (model.DRL.forward, model.py:254-515; recorded by tests/golden/make_golden_actor.py) against one
episode on the MI355X exactly as INTEGRATION sections 2i / 2j write it: a BatchedContainer, EpisodeStepper(expand_dynamic=
False), proj = pointer.project_static(static_encoder(static[:, 1:, :])), fold_decoder + fold_episode once, forward_step per
step from the stepper's own dynamic_bits, decoder_static and decoder_dynamic; grad enabled, the modules in eval mode, ONE
backward() of L = sum_b adv[b] * sum_t tour_logp[b, t].

Teacher-forced: the policy returns the recorded column and keeps log_softmax(logits + log(current_mask)) at it (computed in
float64 from the float32 logits, as the device head computes it).  A free-running tour cannot be compared -- the two rotations
of a square block are the same column, so the two largest masked logits tie exactly.  Every floating quantity is held to
pointer_model.tolerance(e_ref, want) = 4 e_ref + 16 * 2^-24 * max |want| with the fixture's own e_ref (the reference's float32
run against its float64 run) for that step or parameter; what the stepper hands out is compared exactly.  One episode per
fixture, shared by its tests; each prints its worst err / e_ref."""
import numpy as np
import pytest
import torch

import actor_reference_cases as AC
import pointer_model as PM
import policy_head_model as HM
import tap_net_amd as T
from tap_net_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _RecordedTour(object):
    """the policy: the scorer's logits, then the recorded column; keeps what the step saw and its log-probability"""

    def __init__(self, scorer, tour):
        self.scorer, self.tour = scorer, tour                   # tour (steps, B) int64: a step's row is contiguous
        self.logits, self.logp, self.seen = [], [], []

    def __call__(self, step, current_mask, decoder_static, decoder_dynamic, **kw):
        logits = self.scorer(step=step, decoder_static=decoder_static, decoder_dynamic=decoder_dynamic)
        ptr = self.tour[step]
        # model.py:359, 371-372
        logp = torch.log_softmax(logits.double() + torch.log(current_mask.double()), dim=1).gather(1, ptr.unsqueeze(1))[:, 0]
        self.logits.append(logits)
        self.logp.append(logp)
        self.seen.append(tuple(t.detach().clone() for t in (current_mask, decoder_static, decoder_dynamic)))
        return ptr


def _episode(D, ws):
    z = AC.load(D, ws)
    B, n = AC.BATCH[D], AC.N
    st, dy = AC.instances(D)
    static, dynamic = _dev(st), _dev(dy)
    mods, taken = AC.build(z, D)
    assert len(taken) == AC.N_KEYS[D]
    for m in mods.values():
        m.to(DEV)
        assert not m.training
    static_encoder, enc, dec_s, dec_d, pointer = (mods["static_encoder.conv."], mods["dynamic_encoder."], mods["static_decoder.conv."],
                                                  AC.dynamic_decoder(mods), mods["pointer."])
    env = T.BatchedContainer(B, AC.CONTAINER[D], n, "C+P+S-lb-soft", "diff", device=DEV)
    state = {"hh": None, "last_hh": []}

    def scorer(step, decoder_static, decoder_dynamic):
        logits, state["hh"] = pointer.forward_step(state["proj"], sp.dynamic_bits, state["fold"], decoder_static, decoder_dynamic,
                                                   state["hh"])
        state["last_hh"].append(state["hh"])
        return logits
    _lib.variant_hits_reset(DEV)
    with torch.enable_grad():
        sp = T.EpisodeStepper(static, dynamic, env, steps=n, expand_dynamic=False)
        state["proj"] = pointer.project_static(static_encoder(static[:, 1:, :]))
        P, c = pointer.fold_decoder(dec_s, dec_d, combine='cat')
        state["fold"] = pointer.fold_episode(enc, P, c)
        pol = _RecordedTour(scorer, _dev(z["tour_idx"].astype(np.int64).T))
        out = T.run_episode(static, dynamic, pol, 5, 50, stepper=sp, check=False)
        assert sp.dynamic is None
        tour_logp = torch.stack(pol.logp, dim=1)
        assert tuple(tour_logp.shape) == (B, n) and tour_logp.requires_grad
        (_dev(z["adv"]).double() * tour_logp.sum(1)).sum().backward()
    torch.cuda.synchronize()
    hits = {(kind, extra): sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == kind and k[5] == extra)
            for kind in (_lib.TAP_HIT_DECODER, _lib.TAP_HIT_HEIGHTMAP, _lib.TAP_HIT_POINTER) for extra in (0, 1)}
    sp.check()
    cpu = lambda t: t.detach().cpu().numpy()
    return dict(z=z, D=D, ws=ws, B=B, n=n, hits=hits, tour=cpu(out["tour_idx"]), reward=cpu(out["reward"]),
                logits_dev=[t.detach() for t in pol.logits], masks_dev=[s[0] for s in pol.seen], logp_dev=[t.detach() for t in pol.logp],
                logits=[cpu(t).astype(np.float64) for t in pol.logits], last_hh=[cpu(t)[0].astype(np.float64) for t in state["last_hh"]],
                seen=[tuple(cpu(t) for t in s) for s in pol.seen], tour_logp=cpu(tour_logp),
                grads={k: (None if p.grad is None else cpu(p.grad).astype(np.float64)) for k, p in AC.named_parameters(mods).items()})


_RUNS = {}


@pytest.fixture(params=AC.CASES, ids=["%dd-%s" % c for c in AC.CASES])
def run(request):
    """the device episode of one fixture, made once and left unchanged"""
    if request.param not in _RUNS:
        _RUNS[request.param] = _episode(*request.param)
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


def test_every_step_sees_and_gives_what_the_reference_did(run):
    """per step: the stepper's decoder_static, decoder_dynamic and current_mask equal the recorded ones exactly (integers;
    step 0: zeros), logits and last_hh within the rule of that step's e_ref"""
    z, n = run["z"], run["n"]
    assert len(run["logits"]) == n and len(run["last_hh"]) == n and np.array_equal(run["tour"], z["tour_idx"])
    for k in range(n):
        cur, ds, dd = run["seen"][k]
        assert np.array_equal(cur, z["current_mask"][k].astype(np.float32)), k
        assert ds.shape == z["decoder_static"][k].shape and np.array_equal(ds, z["decoder_static"][k].astype(np.float32)), k
        assert dd.size == z["decoder_dynamic"][k].size and \
            np.array_equal(dd.reshape(z["decoder_dynamic"][k].shape), z["decoder_dynamic"][k].astype(np.float32)), k
    label = "actor %dD %s" % (run["D"], run["ws"])
    _held(label, [("logits %d" % k, run["logits"][k], z["logits"][k], z["e_ref_logits"][k]) for k in range(n)] +
          [("last_hh %d" % k, run["last_hh"][k], z["last_hh"][k], z["e_ref_last_hh"][k]) for k in range(n)])


def test_after_the_episode(run):
    """tour_logp under the same rule, the reward within 1e-6 of the reference's -scores (the stepper's check() ran clean
    when the episode was made)"""
    z = run["z"]
    _held("actor %dD %s" % (run["D"], run["ws"]), [("tour_logp", run["tour_logp"], z["tour_logp"], z["e_ref_tour_logp"])])
    err = float(np.abs(run["reward"].astype(np.float64) - z["neg_scores"].astype(np.float64)).max())
    print("actor %dD %s reward: err %.3g" % (run["D"], run["ws"], err))
    assert run["reward"].shape == z["neg_scores"].shape and err <= 1e-6


def test_every_parameters_gradient(run):
    """every key of the reference's state dict has a gradient on the device, the wanted one is non-zero, and the two agree
    within the rule of that parameter's e_ref"""
    z = run["z"]
    keys = sorted(k[len("sd_"):] for k in z if k.startswith("sd_"))
    assert len(keys) == AC.N_KEYS[run["D"]] and sorted(run["grads"]) == keys
    for k in keys:
        assert run["grads"][k] is not None and np.abs(z["grad_" + k]).max() > 0, k
    _held("actor %dD %s gradient" % (run["D"], run["ws"]), [(k, run["grads"][k], z["grad_" + k], z["e_ref_grad_" + k]) for k in keys])


def test_the_kernels_ran(run):
    """n forward launches of this dimension's decoder step and none of the other kind, n of pointer_scores, and the same
    counts backward (the height-map step's backward is decoder_step's launch): the kernels ran, not the torch path"""
    n, hits = run["n"], run["hits"]
    mine, other = (_lib.TAP_HIT_DECODER, _lib.TAP_HIT_HEIGHTMAP) if run["D"] == 2 else (_lib.TAP_HIT_HEIGHTMAP, _lib.TAP_HIT_DECODER)
    assert hits[(mine, 0)] == n and hits[(other, 0)] == 0, hits
    assert hits[(_lib.TAP_HIT_DECODER, 1)] == n and hits[(_lib.TAP_HIT_HEIGHTMAP, 1)] == 0, hits
    assert hits[(_lib.TAP_HIT_POINTER, 0)] == n and hits[(_lib.TAP_HIT_POINTER, 1)] == n, hits


def test_the_head_picks_a_maximum_of_the_reference(run):
    """pointer_pick(logits, current_mask), greedy, on each step's device logits: ties are exact in the reference, so the
    column need not be the recorded one, but the fixture's float64 masked logit at it lies within twice that step's
    tolerance of the row's maximum (each of the two logits may be one tolerance off); where it is the recorded column, the
    head's logp is the kept log-softmax value, an fp32 neighbour.

    Both sides compute log S in float64 with S = the sum of exp(l - max) >= 1, each of its at most nR - 1 additions rounded
    to 2^-53 S; on a peaked row ('sharp': logp down to -1e-9) that absolute error is more than an fp32 neighbour of logp
    itself (seen on the MI355X: -9.4162722e-10 against -9.41626998e-10, one float64 ulp of S apart).  So two values that
    float64 cannot tell apart, 2 (nR - 1) 2^-53 or closer, agree as well; everywhere else the neighbour rule stands"""
    z, B, n = run["z"], run["B"], run["n"]
    ar = np.arange(B)
    resolved = 2.0 * (z["logits"].shape[2] - 1) * 2.0 ** -53
    same, worst = 0, 0.0
    for k in range(n):
        with torch.no_grad():
            ptr, logp = T.pointer_pick(run["logits_dev"][k], run["masks_dev"][k])
        ptr, logp = ptr.cpu().numpy(), logp.cpu().numpy()
        cur = z["current_mask"][k] != 0
        assert cur[ar, ptr].all(), k
        want = np.where(cur, z["logits"][k], -np.inf)
        tol = PM.tolerance(float(z["e_ref_logits"][k]), z["logits"][k])
        short = want.max(axis=1) - want[ar, ptr]
        worst = max(worst, float(short.max()) / tol)
        assert (short <= 2 * tol).all(), (k, float(short.max()), tol)
        rec = ptr == z["tour_idx"][:, k]
        same += int(rec.sum())
        kept = run["logp_dev"][k].cpu().numpy()
        assert kept.dtype == np.float64
        near = HM.neighbour32(logp[rec], kept[rec]) | (np.abs(logp[rec].astype(np.float64) - kept[rec]) <= resolved)
        assert near.all(), (k, logp[rec][~near], kept[rec][~near])
    print("actor %dD %s head: %d of %d picks are the recorded column; worst shortfall / tolerance %.3g" % (
        run["D"], run["ws"], same, B * n, worst))
    assert same > 0
