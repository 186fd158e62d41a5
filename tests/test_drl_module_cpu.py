"""tools.DRL without a GPU: the reference's state dict loads into ONE module, and the module -- teacher-forced, float64, on a
recorded stepper that hands out what the fixture recorded -- is held to the reference's own actor (tests/golden/actor_*.npz,
model.DRL.forward) by the rule tests/test_actor_reference_cpu.py's GPU twin applies to the same quantities:
pointer_model.tolerance(e_ref, want) with the fixture's own e_ref."""
import numpy as np
import pytest
import torch

import actor_reference_cases as AC
import oracle_lib as O
import pointer_model as PM
import tap_net_amd as T
from tap_net_amd import pack


def reference_args(D, decoder_input_type='shape_heightmap', input_type='bot', **kw):
    """the reference's positional arguments for the fixtures' actor (static_size D, dynamic_size 3 n, He 32, Hd 64, W 5, H 50)"""
    args = [D, 3 * AC.N, AC.HE, AC.HD, False, input_type, True, 5, 50, D, "C+P+S-lb-soft", decoder_input_type, "diff", "LB_GREEDY",
            pack.update_dynamic, pack.update_mask]
    return T.DRL(*args, **kw)


class _Env(object):
    def __init__(self, B):
        self.errors = torch.zeros(B, dtype=torch.int32)


class RecordedStepper(object):
    """``pack.EpisodeStepper``'s interface over a fixture: per step the recorded current_mask, decoder_static and
    decoder_dynamic, the 0/1 ``dynamic`` (rebuilt with the oracle) where a stepper has its bit shadow, -neg_scores as the
    ratio; ``step`` checks the module's pick against the recorded tour"""

    def __init__(self, z, D, dtype=torch.float64):
        self.z, self.D, self.dtype = z, D, dtype
        self.steps, self.B = AC.N, AC.BATCH[D]
        self.env = _Env(self.B)
        self.tour = torch.zeros(self.B, self.steps, dtype=torch.int64)
        self.ratio = torch.from_numpy(-z["neg_scores"].astype(np.float64))
        st, dyn = AC.instances(D)
        self._dyn, tour = [dyn], z["tour_idx"].astype(np.int64)
        for k in range(self.steps):
            self._dyn.append(O.update_dynamic(self._dyn[-1], st, tour[:, k], AC.N, 3))
        self.seen = []

    def _hand_out(self, k):
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(self.dtype)
        self.k = k
        self.dynamic_bits = t(self._dyn[k])
        if k < self.steps:
            self.current_mask = t(self.z["current_mask"][k])
            self.decoder_static, self.decoder_dynamic = t(self.z["decoder_static"][k]), t(self.z["decoder_dynamic"][k])

    def begin(self, static, dynamic):
        self.begun = (static, dynamic)
        self._hand_out(0)
        return self

    def step(self, ptr):
        assert np.array_equal(ptr.numpy(), self.z["tour_idx"][:, self.k])
        self.tour[:, self.k] = ptr
        self._hand_out(self.k + 1)


@pytest.mark.parametrize("D,ws", AC.CASES)
def test_the_reference_state_dict_loads_strictly(D, ws):
    """T.DRL(<the reference's arguments>) takes the fixture's whole state dict with strict=True; its own keys are the
    fixture's (16 in 2D, 20 in 3D), with the fixture's shapes"""
    z = AC.load(D, ws)
    sd = AC.state_dict(z)
    actor = reference_args(D)
    actor.load_state_dict(sd, strict=True)
    own = actor.state_dict()
    assert set(own) == set(sd) and len(own) == AC.N_KEYS[D]
    for k, v in sd.items():
        assert torch.equal(own[k], v), k
    assert isinstance(actor.pointer, T.Pointer) and isinstance(actor.dynamic_encoder, T.DynamicBitsEncoder)
    assert isinstance(actor.dynamic_decoder, T.HeightmapEncoder) == (D == 3)


@pytest.mark.parametrize("D", [2, 3])
def test_the_other_decoder_input_types_have_the_references_children(D):
    """model.py:210-222: 'shape_only' -> decoder, an Encoder(static_size, Hd); 'heightmap_only' -> dynamic_decoder alone, an
    Encoder(heightmap_width, Hd) in 2D (width W - 1 for 'diff') and a HeightmapEncoder(2, Hd, (W, W)) in 3D; xavier-uniform on
    every parameter with more than one axis, as the reference initialises"""
    He, Hd = AC.HE, AC.HD
    common = {"static_encoder.conv.weight": (He, D, 1), "static_encoder.conv.bias": (He,),
              "dynamic_encoder.conv.weight": (He, 3 * AC.N, 1), "dynamic_encoder.conv.bias": (He,),
              "pointer.v": (1, 1, Hd), "pointer.W": (1, Hd, 4 * He), "pointer.encoder_attn.v": (1, 1, Hd),
              "pointer.encoder_attn.W": (1, Hd, 2 * He + Hd), "pointer.gru.weight_ih_l0": (3 * Hd, Hd),
              "pointer.gru.weight_hh_l0": (3 * Hd, Hd), "pointer.gru.bias_ih_l0": (3 * Hd,), "pointer.gru.bias_hh_l0": (3 * Hd,)}

    def hm(prefix, m):
        if D == 2:
            return {prefix + "conv.weight": (m, 4, 1), prefix + "conv.bias": (m,)}
        return {prefix + "conv1.weight": (m // 4, 2, 1, 1), prefix + "conv1.bias": (m // 4,), prefix + "conv2.weight": (m // 2, m // 4, 1, 1),
                prefix + "conv2.bias": (m // 2,), prefix + "conv3.weight": (m, m // 2, 2, 2), prefix + "conv3.bias": (m,)}
    want = {"shape_only": dict(common, **{"decoder.conv.weight": (Hd, D, 1), "decoder.conv.bias": (Hd,)}),
            "heightmap_only": dict(common, **hm("dynamic_decoder.", Hd)),
            "shape_heightmap": dict(common, **dict(hm("dynamic_decoder.", Hd // 2), **{"static_decoder.conv.weight": (Hd // 2, D, 1),
                                                                                       "static_decoder.conv.bias": (Hd // 2,)}))}
    for kind, shapes in want.items():
        torch.manual_seed(5)
        actor = reference_args(D, kind)
        assert {k: tuple(v.shape) for k, v in actor.state_dict().items()} == shapes, kind
        for k, p in actor.named_parameters():
            if p.dim() > 1:                 # xavier-uniform: within its bound, and spread over it
                fan_out, fan_in = p.shape[0] * p[0][0].numel(), p.shape[1] * p[0][0].numel()
                bound = float(np.sqrt(6.0 / (fan_in + fan_out)))
                assert 0.5 * bound < float(p.detach().abs().max()) <= bound, (kind, k)
    # the full height-map ('zero' is not 'diff'): W columns, one map
    sd = T.DRL(2, 30, AC.HE, AC.HD, False, 'bot', True, 5, 50, 2, "C+P+S-lb-soft", 'heightmap_only', 'full', "LB_GREEDY", None, None,
               unit=1).state_dict()
    assert tuple(sd["dynamic_decoder.conv.weight"].shape) == (AC.HD, 5, 1)


def test_unsupported_arguments_raise():
    for input_type in ('mul', 'mul-with', 'use-pnet'):
        with pytest.raises(NotImplementedError, match=input_type):
            reference_args(2, input_type=input_type)
    args = [2, 30, AC.HE, AC.HD, False, 'bot', True, 5, 50, 2, "C+P+S-lb-soft", 'shape_heightmap', "diff", "LB_GREEDY"]
    with pytest.raises(NotImplementedError):
        T.DRL(*args, lambda *a: None, None)
    with pytest.raises(NotImplementedError):
        T.DRL(*args, None, lambda *a: None)
    assert T.DRL(*args, None, None, 1, 0.1, 1, seed=3, env_offset=7, fold='proj').pointer.drop_rnn.p == 0.1
    with pytest.raises(TypeError):
        T.DRL(*args, None, None, 1, 0.1, 1, 3)                  # seed is keyword-only
    assert T.tools.DRL is T.DRL


_RUNS = {}


def _run(D, ws):
    """the module's teacher-forced float64 episode on the recorded stepper, made once per fixture"""
    if (D, ws) in _RUNS:
        return _RUNS[(D, ws)]
    z = AC.load(D, ws)
    actor = reference_args(D)
    actor.load_state_dict(AC.state_dict(z), strict=True)
    actor.double().eval()
    st, dyn = AC.instances(D)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    sp = RecordedStepper(z, D)
    logits, last_hh = [], []
    step = actor.pointer._forward_step

    def spy(*a):                                                # the per-step logits and last_hh, which forward does not return
        out = step(*a)
        logits.append(out[0].detach().numpy())
        last_hh.append(out[1].detach().numpy()[0])
        return out
    actor.pointer._forward_step = spy
    tour_idx, tour_logp, none, reward = actor(t(st), t(dyn), (t(z["decoder_static"][0]), t(z["decoder_dynamic"][0])),
                                              tour=torch.from_numpy(z["tour_idx"].astype(np.int64)), stepper=sp)
    (t(z["adv"]) * tour_logp.sum(1)).sum().backward()
    grads = {k: p.grad.numpy() for k, p in actor.named_parameters()}
    _RUNS[(D, ws)] = dict(z=z, out=(tour_idx, tour_logp, none, reward), logits=logits, last_hh=last_hh, grads=grads)
    return _RUNS[(D, ws)]


def _held(label, rows):
    worst = 0.0
    for name, got, want, e in rows:
        want = np.asarray(want, np.float64)
        assert got.shape == want.shape and np.isfinite(got).all(), name
        err, tol = float(np.abs(got - want).max()), PM.tolerance(float(e), want)
        worst = max(worst, AC.ratio(err, float(e)))
        assert np.abs(want).max() > 0 and err <= tol, (label, name, err, tol)
    print("%s: worst err / e_ref %.3g" % (label, worst))


@pytest.mark.parametrize("D,ws", AC.CASES)
def test_teacher_forced_module_gives_the_references_numbers(D, ws):
    """logits and last_hh per step, tour_logp, the tuple forward returns"""
    r = _run(D, ws)
    z, n = r["z"], AC.N
    tour_idx, tour_logp, none, reward = r["out"]
    assert none is None and tour_logp.dtype is torch.float64 and tuple(tour_logp.shape) == (AC.BATCH[D], n)
    assert np.array_equal(tour_idx.numpy(), z["tour_idx"]) and np.array_equal(reward.numpy(), z["neg_scores"].astype(np.float64))
    assert len(r["logits"]) == n
    _held("DRL cpu %dD %s" % (D, ws),
          [("logits %d" % k, r["logits"][k], z["logits"][k], z["e_ref_logits"][k]) for k in range(n)] +
          [("last_hh %d" % k, r["last_hh"][k], z["last_hh"][k], z["e_ref_last_hh"][k]) for k in range(n)] +
          [("tour_logp", tour_logp.detach().numpy(), z["tour_logp"], z["e_ref_tour_logp"])])


@pytest.mark.parametrize("D,ws", AC.CASES)
def test_teacher_forced_module_gives_the_references_gradients(D, ws):
    """every parameter's gradient of sum_b adv[b] sum_t tour_logp[b, t]"""
    r = _run(D, ws)
    z = r["z"]
    keys = sorted(k[len("sd_"):] for k in z if k.startswith("sd_"))
    assert sorted(r["grads"]) == keys
    _held("DRL cpu %dD %s gradient" % (D, ws), [(k, r["grads"][k], z["grad_" + k], z["e_ref_grad_" + k]) for k in keys])


def test_free_running_on_the_cpu_draws_from_the_modules_source():
    """train(): the picks come from the module's StepDropout through rollout.pick_uniforms -- torch's generator is not
    touched, the episode counter advances per call, and every pick is selectable; eval(): greedy"""
    z = AC.load(2, "init")
    actor = reference_args(2, seed=17)
    actor.load_state_dict(AC.state_dict(z), strict=True)
    actor.double()
    st, dyn = AC.instances(2)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))

    class Free(RecordedStepper):                                # hands out the recorded masks whatever is picked
        def step(self, ptr):
            assert bool((self.current_mask.gather(1, ptr.unsqueeze(1)) == 1).all())
            self.tour[:, self.k] = ptr
            self._hand_out(self.k + 1)
    before = torch.random.get_rng_state()
    tours = []
    for mode in (actor.train, actor.train, actor.eval, actor.eval):
        mode()
        sp = Free(z, 2)
        with torch.no_grad():
            out = actor(t(st), t(dyn), (t(z["decoder_static"][0]), t(z["decoder_dynamic"][0])), stepper=sp)
        assert out[0] is sp.tour and bool(torch.isfinite(out[1]).all())
        tours.append(sp.tour.clone())
    assert torch.equal(before, torch.random.get_rng_state())
    assert not torch.equal(tours[0], tours[1]) and torch.equal(tours[2], tours[3])
    assert actor.step_dropout("cpu").state.tolist() == [17, 2] and actor.step_dropout("cpu").pick == AC.N
