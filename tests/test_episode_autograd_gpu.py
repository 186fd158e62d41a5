"""What a trainer does, on the MI355X: n decoding steps with a network between them, then ONE backward() through all of
them -- against the float64 loop of tests/episode_actor_model.py on env tensors re-derived with the oracle.

The step objects' launches write their buffers through raw pointers: torch's version counters never move, so a
convolution that saved a stepper's view for its weight gradient would read what LATER steps wrote, without an error.
Three groups of tests:
  * nothing handed to a policy changes under it while grad is enabled (every loop of rollout / rolling), and under
    no_grad the steppers keep handing out their own buffers (no copy: the host step and the graph captures stay as they are);
  * a whole training step on three paths -- the float path on the default stepper as INTEGRATION section 2c writes it (2D
    and the two-plane 3D window), and the lean path on the bit shadow -- within pointer_model.tolerance(e_ref, want) of
    the float64 loop for tour_logp and EVERY parameter's gradient, e_ref being the float32 CPU loop's own error;
  * ``inplace_dynamic=True``: one tensor by contract; a backward through a network that saved it raises.
Each gradient test prints err / e_ref per parameter."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import episode_actor_model as A
import pointer_model as PM
import tap_net_amd as T
from tap_net_amd import _lib, synth
from test_dyn_encoder_gpu import _window

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RNN_RT = 'C+P+S-G-soft'


# ---- nothing handed to a policy changes under it ---------------------------------------------------------------------
class _Keep(object):
    """wraps a policy (or a pack policy): keeps every tensor it was handed and a clone of it"""

    def __init__(self, inner):
        self.inner, self.kept, self.calls = inner, [], 0

    def _keep(self, name, t):
        if torch.is_tensor(t):
            self.kept.append((self.calls, name, t, t.clone()))

    def __call__(self, *args, **kw):
        for i, t in enumerate(args):
            self._keep("arg%d" % i, t)
        for name, t in kw.items():
            self._keep(name, t)
        self.calls += 1
        return self.inner(*args, **kw)

    def changed(self):
        """[(call, name)] of the kept tensors that no longer hold the bytes they held when they were handed out"""
        torch.cuda.synchronize()
        return [(call, name) for call, name, t, c in self.kept
                if t.shape != c.shape or not torch.equal(t.contiguous().view(torch.uint8), c.contiguous().view(torch.uint8))]


def _c2(B, seed):
    static, dynamic = synth.rand_instances(B, 10, 2, seed=seed)
    tape = synth.random_feasible_tape(static, dynamic, 10, seed=seed + 1)
    return static.to(DEV).contiguous(), dynamic.to(DEV).contiguous(), tape.to(DEV)


def _seam_stepper(D):
    n, static, dynamic, cs = _window(D)
    tape = synth.random_feasible_tape(static.cpu(), dynamic.cpu(), n, seed=7).to(DEV)
    pol = _Keep(T.TapePolicy(tape))
    out = T.run_episode(static, dynamic, pol, cs[0], cs[-1], check=False)
    assert "stepper" in out and torch.equal(out["tour_idx"], tape)
    assert int(dynamic.shape[1]) == (30 if D == 2 else 66)
    return [pol], n


def _seam_unfused(fused):
    """fused=False: MaskStepper + add_new_blocks_gather; fused=True with bits=False: the EnvTransition loop"""
    static, dynamic, tape = _c2(64, 11)
    pol = _Keep(T.TapePolicy(tape))
    out = T.run_episode(static, dynamic, pol, 5, 50, fused=fused, bits=False, check=False)
    assert "stepper" not in out and torch.equal(out["tour_idx"], tape)
    return [pol], 10


def _seam_rolling():
    """RollingStepper + EpisodeStepper through run_rolling_episode at (2D, N = 30, child = 4), the smallest window of
    test_rolling_episode_vs_oracle; the tour is recorded under no_grad with a random feasible policy first"""
    from tap_net_amd import generate as gen
    D, N, child, init, B = 2, 30, 4, [7, 200], 64
    _, _, blocks, positions = gen.generate_instances(B, N, D, init[0], init[-1], 1, (1, 5), seed=3, device=DEV, return_aux=True)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    H = 4 * N + 10
    with torch.no_grad():
        first = T.run_rolling_episode(blocks, positions, init, lambda current_mask, **_: torch.multinomial(current_mask, 1, generator=g).squeeze(1),
                                      5, H, child_graph_size=child)
    tour = first["tour_idx"].clone()
    pol = _Keep(T.TapePolicy(tour))
    out = T.run_rolling_episode(blocks, positions, init, pol, 5, H, child_graph_size=child)
    assert "steppers" in out and torch.equal(out["tour_idx"], tour) and torch.equal(out["nodes"], first["nodes"])
    assert torch.equal(out["reward"].nan_to_num(), first["reward"].nan_to_num())
    return [pol], N


def _seam_pack_policy():
    static, dynamic, tape = _c2(64, 13)
    xs = torch.as_tensor(np.random.RandomState(4).randint(0, 5, (64, 10)), device=DEV)
    pol = _Keep(T.TapePolicy(tape))
    pack_pol = _Keep(lambda pin, blk: xs[:, pack_pol.calls - 1])
    out = T.run_episode(static, dynamic, pol, 5, 60, reward_type='C+P+S-SL-soft', heightmap_type='diff', pack_policy=pack_pol)
    assert torch.equal(out["place_x"], xs) and pack_pol.calls == 10
    return [pol, pack_pol], 10


def _seam_rnn_loop():
    """rollout.rnn_loop: decoder_dynamic is PackEngines.get_heightaps after the pack-net's forward"""
    static, dynamic, tape = _c2(64, 17)
    torch.manual_seed(9)
    net = T.tools.PackRNN(2, 32, 5, 32, 5, 60, 'diff', pack_net_type='G').to(DEV).eval()
    pol = _Keep(T.TapePolicy(tape))
    out = T.run_episode(static, dynamic, pol, 5, 60, reward_type=RNN_RT, heightmap_type='diff', pack_rnn=net)
    assert torch.equal(out["tour_idx"], tape) and out["pack_logp"].requires_grad
    return [pol], 10


SEAMS = {"stepper-2d": lambda: _seam_stepper(2), "stepper-3d": lambda: _seam_stepper(3),
         "mask-stepper": lambda: _seam_unfused(False), "env-transition": lambda: _seam_unfused(True),
         "rolling-steppers": _seam_rolling, "pack-policy": _seam_pack_policy, "rnn-loop": _seam_rnn_loop}


@pytest.mark.parametrize("seam", sorted(SEAMS))
def test_nothing_handed_to_a_policy_changes_while_grad_is_enabled(seam):
    with torch.enable_grad():
        keeps, steps = SEAMS[seam]()
    for keep in keeps:
        assert keep.calls == steps and len(keep.kept) >= 2 * steps
        changed = keep.changed()
        assert not changed, "%s: %d of %d kept tensors changed after they were handed out, first %s" % (
            seam, len(changed), len(keep.kept), changed[:6])


def test_under_no_grad_the_steppers_hand_out_their_own_buffers():
    """no copy and no torch op under no_grad: the attributes ARE the buffers the launches write -- also on a stepper that
    has run with grad enabled before"""
    static, dynamic, tape = _c2(64, 19)
    env = T.BatchedContainer(64, [5, 50], 10, "C+P+S-lb-soft", "diff", device=DEV)
    sp = T.EpisodeStepper(static, dynamic, env)
    flen = int(np.prod(env._feature_shape()[1:]))

    def own():
        assert sp.decoder_dynamic.data_ptr() == sp._dec.data_ptr()
        assert sp.decoder_static.data_ptr() == sp._dec.data_ptr() + 64 * flen * 4

    for first in (torch.no_grad, torch.enable_grad, torch.no_grad):
        with first():
            sp.begin(static, dynamic)
            sp.step(tape[:, 0].contiguous())
        with torch.no_grad():
            sp.begin(static, dynamic)
            assert sp.current_mask is sp._views[1][1] and sp.mask is sp._views[1][2] and sp.dynamic is dynamic
            own()
            for t in range(3):
                w = sp.step(tape[:, t].contiguous())
                assert sp.dynamic is sp._views[w][0] and sp.current_mask is sp._views[w][1] and sp.mask is sp._views[w][2]
                assert sp.dynamic_bits is sp._bits[w]
                own()
    with torch.enable_grad():                                      # and with grad enabled they are not
        sp.begin(static, dynamic)
        w = sp.step(tape[:, 0].contiguous())
        assert sp.dynamic_bits is sp._bits[w]                      # the shadow stays the buffer: the autograd functions clone it
        for mine, buf in ((sp.dynamic, sp._views[w][0]), (sp.current_mask, sp._views[w][1]), (sp.mask, sp._views[w][2]),
                          (sp.decoder_dynamic, sp._dec)):
            assert torch.equal(mine.reshape(-1), buf.reshape(-1)[:mine.numel()])
            assert mine.untyped_storage().data_ptr() != buf.untyped_storage().data_ptr()


def test_inplace_dynamic_with_grad_enabled_fails_loudly():
    """``inplace_dynamic=True`` keeps ONE fp32 tensor for the episode.  Under no_grad that is its purpose; with grad enabled
    a step marks the tensor as modified, so the backward of a network that saved it raises autograd's RuntimeError
    instead of computing a weight gradient from a later step's values; a loop that saves nothing is not disturbed"""
    static, dynamic, tape = _c2(64, 23)
    env = T.BatchedContainer(64, [5, 50], 10, "C+P+S-lb-soft", "diff", device=DEV)
    sp = T.EpisodeStepper(static, dynamic, env, inplace_dynamic=True)
    torch.manual_seed(1)
    conv = nn.Conv1d(30, 8, 1).to(DEV)
    with torch.enable_grad():
        sp.begin(static, dynamic)
        sp.step(tape[:, 0].contiguous())
        assert sp.dynamic is sp._dyn[0]
        hidden = conv(sp.dynamic)
        sp.step(tape[:, 1].contiguous())
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            hidden.sum().backward()
        # a backward BEFORE the next step wrote the tensor is the true gradient: sum over (b, c) of dynamic[b, r, c]
        conv.zero_grad()
        sp.step(tape[:, 2].contiguous())
        want = sp.dynamic.sum((0, 2))[None, :, None].expand(8, -1, -1).clone()
        conv(sp.dynamic).sum().backward()
        assert float(want.abs().max()) > 0 and torch.allclose(conv.weight.grad, want)
        for t in range(3, 10):
            sp.step(tape[:, t].contiguous())
    with torch.no_grad():
        out = T.run_episode(static, dynamic, T.TapePolicy(tape), 5, 50, stepper=sp, check=False)
    assert out["dynamic"] is sp._dyn[0] and not bool(out["dynamic"].any())


# ---- a whole training step -------------------------------------------------------------------------------------------
N_STEPS = {2: 10, 3: 22}


def _setup(D, seed):
    """B = 67 instances of the 2D c2 window (n = 10: rows 30, nR 20) or of the two-plane 3D window (n = 22: rows 66, nR 132),
    the actor, and the pre-drawn u (n, B), adv (B,) and ghh (1, B, H)"""
    B, n = 67, N_STEPS[D]
    cs = [5, 50] if D == 2 else [5, 5, 200]
    static, dynamic = synth.rand_instances(B, n, D, seed=seed)
    rng = np.random.RandomState(seed + 1)
    u = rng.rand(n, B).astype(np.float32)
    adv = rng.randn(B).astype(np.float32)
    ghh = rng.randn(1, B, A.H).astype(np.float32)
    flen = (cs[0] - 1) if D == 2 else 2 * cs[0] * cs[1]
    actor = A.make_actor(static, dynamic, flen, seed + 2)
    return dict(B=B, n=n, D=D, cs=cs, static=static, dynamic=dynamic, u=u, adv=adv, ghh=ghh, actor=actor)


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _loss_backward(S, tour_logp, hh):
    assert tuple(tour_logp.shape) == (S["B"], S["n"]) and tour_logp.requires_grad
    loss = (_to(S["adv"]) * tour_logp.sum(1)).sum() + (hh * _to(S["ghh"])).sum()
    loss.backward()


def _float_path(S):
    """INTEGRATION section 2c as written: the network reads the default stepper's attributes"""
    net = copy.deepcopy(S["actor"]).to(DEV).train()
    static, dynamic, u = S["static"].to(DEV).contiguous(), S["dynamic"].to(DEV).contiguous(), _to(S["u"])
    env = T.BatchedContainer(S["B"], S["cs"], S["n"], "C+P+S-lb-soft", "diff", device=DEV)
    with torch.enable_grad():
        sp = T.EpisodeStepper(static, dynamic, env)
        sp.begin(static, dynamic)
        static_hidden = net.static_encoder(static)
        hh = torch.zeros(1, S["B"], A.H, device=DEV)
        logps = []
        for k in range(S["n"]):
            dec = net.decoder_input(sp.decoder_static, sp.decoder_dynamic)
            logits, hh = net.pointer(static_hidden, net.dynamic_encoder(sp.dynamic), dec, hh)
            ptr, logp = T.pointer_pick(logits, sp.current_mask, u[k])
            logps.append(logp.unsqueeze(1))
            sp.step(ptr)
        tour_logp = torch.cat(logps, dim=1)
        _loss_backward(S, tour_logp, hh)
    sp.check()
    return sp.tour.cpu().numpy(), tour_logp.detach().double().cpu().numpy(), A.named_grads(net)


def _lean_path(S):
    """the bit shadow end to end: no fp32 ``dynamic``, proj once per episode, forward_bits per step, the head as a policy"""
    net = copy.deepcopy(S["actor"]).to(DEV).train()
    static, dynamic, u = S["static"].to(DEV).contiguous(), S["dynamic"].to(DEV).contiguous(), _to(S["u"])
    env = T.BatchedContainer(S["B"], S["cs"], S["n"], "C+P+S-lb-soft", "diff", device=DEV)
    state = {}

    def scorer(step, decoder_static, decoder_dynamic, **_):
        dec = net.decoder_input(decoder_static, decoder_dynamic)
        logits, state["hh"] = net.pointer.forward_bits(state["proj"], sp.dynamic_bits, net.dynamic_encoder, dec, state["hh"])
        return logits
    _lib.variant_hits_reset(DEV)
    with torch.enable_grad():
        sp = T.EpisodeStepper(static, dynamic, env, expand_dynamic=False)
        state["proj"] = net.pointer.project_static(net.static_encoder(static))
        state["hh"] = torch.zeros(1, S["B"], A.H, device=DEV)
        pol = T.PointerHeadPolicy(scorer, u=u)
        out = T.run_episode(static, dynamic, pol, S["cs"][0], S["cs"][-1], stepper=sp, check=False)
        assert sp.dynamic is None
        tour_logp = pol.tour_logp()
        _loss_backward(S, tour_logp, state["hh"])
    sp.check()
    hits = {extra: sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == _lib.TAP_HIT_POINTER and k[5] == extra)
            for extra in (0, 1)}
    assert hits == {0: S["n"], 1: S["n"]}, hits                    # the kernel ran: n forward and n backward launches
    return out["tour_idx"].cpu().numpy(), tour_logp.detach().double().cpu().numpy(), A.named_grads(net)


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))


def _against_the_float64_loop(path, S, tour, logp, grads, check=True):
    """the device run's tour, teacher-forced through the CPU loop in float64 (wanted) and float32 (e_ref) on env tensors
    the oracle re-derives -> {name: (got, want, tolerance)}, after asserting every one of them unless ``check`` is False
    (the caller then only wants the tolerances)"""
    st, dy = S["static"].numpy(), S["dynamic"].numpy()
    env = A.episode_tensors(st, dy, tour, S["cs"])
    ar = np.arange(S["B"])
    assert all((env["current_mask"][k][ar, tour[:, k]] == 1).all() for k in range(S["n"]))     # the device's picks are selectable
    logp64, want = A.train_step(S["actor"], torch.float64, st, env, tour, S["adv"], S["ghh"])
    logp32, ref32 = A.train_step(S["actor"], torch.float32, st, env, tour, S["adv"], S["ghh"])
    assert sorted(grads) == sorted(want) and len(want) == 8 + 4 * 2
    rows = [("tour_logp", logp, logp64, logp32)] + [(name, grads[name], want[name], ref32[name]) for name in sorted(want)]
    out, failed, worst = {}, [], ("", 0.0)
    for name, got, w, r in rows:
        assert got.shape == w.shape and np.isfinite(got).all() and np.isfinite(w).all(), name
        e, err = float(np.abs(r - w).max()), float(np.abs(got - w).max())
        tol = PM.tolerance(e, w)
        print("%s %s: err %.3g e_ref %.3g ratio %.2f tolerance %.3g max|want| %.3g" % (path, name, err, e, _ratio(err, e), tol,
                                                                                      np.abs(w).max()))
        if not (np.abs(w).max() > 0 and err <= tol):
            failed.append((name, err, tol))
        if _ratio(err, e) > worst[1]:
            worst = (name, _ratio(err, e))
        out[name] = (got, w, tol)
    print("%s: worst err / e_ref %.2f (%s)" % (path, worst[1], worst[0]))
    assert not (check and failed), (path, failed)
    return out


@pytest.fixture(scope="module")
def c2_setup():
    return _setup(2, 41)


@pytest.fixture(scope="module")
def c2_runs(c2_setup):
    """the two device runs of the shared seed, made once: {path: (tour, tour_logp, grads)}"""
    return {"float": _float_path(c2_setup), "lean": _lean_path(c2_setup)}


def test_training_step_on_the_default_stepper(c2_setup, c2_runs):
    """path a: Conv1d on sp.dynamic / sp.decoder_static / sp.decoder_dynamic, Pointer.forward, pointer_pick(logits,
    sp.current_mask, u[k]), one backward().  Before the steppers handed out copies under grad (seed 41, on the MI355X) the
    three encoder weights that save a stepper view missed the float64 gradient by 4.1e5 (dynamic), 2.7e5 (decoder_static)
    and 4.0e5 (decoder_dynamic) times the tolerance, with tour_logp right; with the copies they are at 0.8, 1.0 and 0.8 x
    e_ref.

    The smallest gradients here, pointer.encoder_attn.W / .v (1e-4 of the largest), see the logits only through the
    context that all columns share, so they read any residue in the row sums of the head's dlogits: with the picked column
    written as g (1 - p[ptr]) they were 5.54 / 4.63 x e_ref off, outside the bound; with the head's zero-sum rows
    (policy.hip: k_policy_pick_backward) 3.72 / 3.22 x."""
    _against_the_float64_loop("float path 2D", c2_setup, *c2_runs["float"])


def test_training_step_on_the_bit_shadow(c2_setup, c2_runs):
    """path b: EpisodeStepper(expand_dynamic=False), DynamicBitsEncoder folded into forward_bits, project_static once,
    PointerHeadPolicy(scorer, u=u) in run_episode, tour_logp().  Pins the cloned shadow, proj's gradient accumulated over
    the n steps through the transposed view, the head's saved probs and n + n pointer launches"""
    _against_the_float64_loop("lean path 2D", c2_setup, *c2_runs["lean"])


def test_the_two_paths_agree(c2_setup, c2_runs):
    """the same seed, actor and uniforms on both paths: equal tours, and every parameter's two gradients within the sum
    of the two paths' tolerances of each other (each path against float64 is the two tests above)"""
    S = c2_setup
    (tour_a, logp_a, grads_a), (tour_b, logp_b, grads_b) = c2_runs["float"], c2_runs["lean"]
    assert np.array_equal(tour_a, tour_b)
    a = _against_the_float64_loop("float path 2D", S, tour_a, logp_a, grads_a, check=False)
    b = _against_the_float64_loop("lean path 2D", S, tour_b, logp_b, grads_b, check=False)
    bad = []
    for name in sorted(a):
        diff = float(np.abs(a[name][0] - b[name][0]).max())
        print("float against lean path, %s: differ by %.3g, tolerances %.3g + %.3g" % (name, diff, a[name][2], b[name][2]))
        if not diff <= a[name][2] + b[name][2]:
            bad.append((name, diff, a[name][2], b[name][2]))
    assert not bad, bad


def test_training_step_on_the_3d_window():
    """path c: path a on the two-plane window (n = 22: rows 66, nR 132; a (2, 5, 5) feature as decoder_dynamic)"""
    S = _setup(3, 63)
    assert tuple(S["dynamic"].shape) == (67, 66, 132)
    _against_the_float64_loop("float path 3D", S, *_float_path(S))
