"""tools.RollingDRL and the fused pointer launch without a GPU.

The reference's rolling actor (tests/golden/rolling_actor_2d.npz: rolling.DRL in rolling.validate's loop, five instances of
20 blocks, windows of 10) against the module in ``double()``: a replay pair stands in for the steppers -- it hands out the
per-step inputs the reference's forward saw and asserts every pick equals the recorded one --, and the module must give the
recorded ``logits`` and ``last_hh`` of every step and ``tour_logp`` to 1e-10, teacher-forced (GIVEN) and free-running
(greedy: the float64 greedy run IS the recorded tour).  Besides: the numpy model of the fused launch on hand cases, the
constructor's parameter list against the recorded one, the refusals, ``StaticFold.with_rows``, and the C entry's argument
checks through the ABI with a null context."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import rolling_actor_model as RM
import tap_net_amd as T
from tap_net_amd import _lib, pack, rollout, tools

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rolling_actor_2d.npz")
B, N, CHILD, R, D, HE, HD = 5, 20, 10, 2, 2, 32, 64


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _state_dict(z):
    return {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")}


def _actor(z=None, **kw):
    actor = T.RollingDRL(D, 3 * CHILD, HE, HD, False, 'bot', True, 5, 100, D, "C+P+S-lb-soft", 'shape_heightmap', "diff", "LB_GREEDY",
                         None, pack.update_dynamic, pack.update_mask, 1, 0.1, 1, **kw)
    if z is not None:
        actor.load_state_dict(_state_dict(z), strict=True)
    return actor


class _Windows(object):
    """what RollingDRL reads of a RollingWindows"""
    B, N, D, child, R, device = B, N, D, CHILD, R, torch.device("cpu")


class _Env(object):
    errors = torch.zeros(B, dtype=torch.int32)

    def reset(self):
        pass


class _Replay(object):
    """Both steppers of rolling._run_rolling_steppers at once: after ``begin`` and after every ``step`` the attributes are what
    the reference's forward saw at that step of the fixture; ``step(ptr)`` asserts the recorded pick"""
    expand_dynamic, _dynamic, dynamic = False, None, None

    def __init__(self, z, dtype=torch.float64):
        self.z, self.dtype, self.env, self.k = z, dtype, _Env(), -1
        self._ones = torch.ones(B, CHILD * R, dtype=dtype)
        self.mask = self._ones
        self.tour = torch.zeros(B, N, dtype=torch.int64)
        self.picked = torch.zeros(B, N, dtype=torch.int32)
        self.ratio = torch.from_numpy(z["ratio"])
        self._dec = None
        self.handed_over = False

    def _at(self, name, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(self.z[name][:, min(self.k, N - 1)])).to(self.dtype if dtype is None else dtype)

    static = property(lambda s: s._at("static"))
    bits = dynamic_bits = property(lambda s: s._at("bits", torch.int64))
    current_mask = property(lambda s: s._at("current_mask"))
    decoder_static = property(lambda s: s._at("decoder_static"))
    decoder_dynamic = property(lambda s: s._at("decoder_dynamic"))

    @property
    def nodes(self):                         # the last graph's node list is what its picks index: rebuilt from the recorded ids
        out = torch.zeros(B, CHILD, dtype=torch.int32)
        ids = torch.from_numpy(self.z["nodes"][:, N - CHILD:].astype(np.int32))
        out.scatter_(1, torch.from_numpy(self.z["tour_idx"][:, N - CHILD:].astype(np.int64)) % CHILD, ids)
        return out

    def begin(self, rw):
        self.k = 0

    def is_last_graph(self):
        return self.k >= N - CHILD

    def begin_shadow(self, static, dynamic, bits, current_mask=None, keep_container=False):
        assert self.k == N - CHILD and keep_container and dynamic is None
        self.handed_over = True

    def load_decoder_inputs(self, dec):
        pass

    def step(self, ptr):
        want = torch.from_numpy(self.z["tour_idx"][:, self.k].astype(np.int64))
        assert torch.equal(ptr.cpu(), want), (self.k, ptr, want)
        assert self.handed_over == (self.k >= N - CHILD)
        self.tour[:, self.k] = ptr
        if self.k < N - CHILD:
            self.picked[:, self.k] = torch.from_numpy(self.z["nodes"][:, self.k].astype(np.int32))
        self.k += 1


def test_model_of_the_fused_launch_on_hand_cases():
    """one hidden row, one static row, no set bit: logits[c] = vp tanh(g1 + G1 xs[c] + k1 + t) with t = sum attn (g2 + G2 xs + k2);
    then the head's rules: greedy takes the first largest selectable logit, an all-masked row is (0, NaN)"""
    Hd, S, nR, rows = 1, 1, 4, 3
    xs = np.array([[[1.0, 2.0, 3.0, 2.0]], [[1.0, 1.0, 1.0, 1.0]], [[4.0, 3.0, 2.0, 1.0]]])
    G = np.array([[0.0], [0.5], [0.0]])
    g = k = np.zeros(3)
    M = np.zeros((3, rows))
    dyn = np.zeros((3, rows, nR), bool)
    q = np.zeros((3, Hd))
    va, vp = np.ones(Hd), np.ones(Hd)
    mask = np.array([[1, 1, 1, 1], [0, 0, 0, 0], [0, 1, 0, 1]], np.float32)
    ptr, logp, logits = RM.fused(xs, G, g, dyn, M, k, q, va, vp, mask)
    assert np.allclose(logits, np.tanh(0.5 * xs[:, 0, :]), atol=1e-15)           # t = 0: segment 2 is all zeros
    assert ptr.tolist() == [2, 0, 1] and np.isnan(logp[1]) and np.isfinite(logp[[0, 2]]).all()
    w = np.exp(logits[0] - logits[0].max())
    assert abs(logp[0] - np.log(w[2] / w.sum())) <= 1e-15
    w = np.exp(logits[2, [1, 3]] - logits[2, 1])
    assert abs(logp[2] - np.log(w[0] / w.sum())) <= 1e-15
    # a set row adds M's column; a tie goes to the first column
    M[1, 0] = 10.0
    dyn[0, 0, 1] = True
    p2, _, l2 = RM.fused(xs, G, g, dyn, M, k, q, va, vp, mask)
    assert p2[0] == 1 and abs(l2[0, 1] - np.tanh(11.0)) <= 1e-15 and np.array_equal(l2[1:], logits[1:])
    flat = RM.fused(np.ones_like(xs), G, g, np.zeros_like(dyn), np.zeros_like(M), k, q, va, vp, mask)
    assert flat[0].tolist() == [0, 0, 1]
    # DRAW: the pick is a selectable column and an all-masked row stays (0, NaN)
    pd, ld, _ = RM.fused(xs, G, g, dyn, M, k, q, va, vp, mask, draw=(7, 1, 2, 3))
    assert pd[1] == 0 and np.isnan(ld[1]) and mask[0, pd[0]] == 1 and mask[2, pd[2]] == 1
    # the GPU comparison's masks: the forced rows are empty and no other row is
    m = RM.random_mask(19, 20, 5)
    assert not m[list(RM.EMPTY_ROWS)].any() and all(m[b].any() for b in range(19) if b not in RM.EMPTY_ROWS)


def test_fixture_loads_strictly_and_the_constructor_is_the_references(z):
    actor = _actor(z)
    assert len(actor.state_dict()) == 16 and isinstance(actor, T.DRL) and T.RollingDRL is tools.RollingDRL
    params = list(inspect.signature(T.RollingDRL.__init__).parameters.values())[1:]
    ref = [str(v) for v in z["ctor_params"]]
    assert [p.name for p in params[:len(ref)]] == ref and ref.index("containers") == ref.index("packing_strategy") + 1
    assert ref.index("update_fn") == ref.index("containers") + 1
    extra = params[len(ref):]
    assert [p.name for p in extra] == ["seed", "env_offset", "fused_pick"] and all(p.kind is p.KEYWORD_ONLY for p in extra)
    assert actor.fused_pick is True and _actor(fused_pick=False).fused_pick is False
    # model.DRL's list is this one without `containers`
    drl = [p.name for p in list(inspect.signature(T.DRL.__init__).parameters.values())[1:]]
    assert [n for n in ref if n != "containers"] == drl[:len(ref) - 1]
    _actor(None)                                             # `containers` is accepted and ignored, whatever it is
    T.RollingDRL(D, 3 * CHILD, HE, HD, False, 'bot', True, 5, 100, D, "C+P+S-lb-soft", 'shape_heightmap', "diff", "LB_GREEDY",
                 [object()], None, None)


def test_refusals():
    for bad in ('mul', 'mul-with', 'use-pnet'):
        with pytest.raises(NotImplementedError):
            T.RollingDRL(D, 3 * CHILD, HE, HD, False, bad, True, 5, 100, D, "C+P+S-lb-soft", 'shape_heightmap', "diff", "LB_GREEDY",
                         None, None, None)
    with pytest.raises(NotImplementedError):
        T.RollingDRL(D, 3 * CHILD, HE, HD, False, 'bot', True, 5, 100, D, "C+P+S-lb-soft", 'shape_heightmap', "diff", "LB_GREEDY",
                     None, lambda *a: None, None)
    actor = _actor().double().eval()

    class Wide(_Windows):
        child = 22                                           # 66 rows: no one-word shadow
    with pytest.raises(ValueError, match="3 \\* child <= 64"):
        actor(Wide(), steppers=(None, None))

    class Odd(_Windows):
        child, R = 5, 6                                      # 30 columns: not a multiple of 4
        D = 3
    with pytest.raises(ValueError, match="multiple of 4"):
        actor(Odd(), steppers=(None, None))
    with pytest.raises(ValueError, match="steppers="):       # off the GPU the module has no steppers of its own
        actor(_Windows())
    with pytest.raises(ValueError, match="tour must be"):
        actor(_Windows(), steppers=(None, None), tour=torch.zeros(B, N - 1, dtype=torch.int64))


@pytest.mark.parametrize("forced", [True, False], ids=["given", "greedy"])
@pytest.mark.parametrize("fused_pick", [True, False])
def test_float64_module_reproduces_the_reference(z, forced, fused_pick):
    actor = _actor(z, fused_pick=fused_pick).double().eval()
    rp = _Replay(z)
    tour = torch.from_numpy(z["tour_idx"].astype(np.int64)) if forced else None
    tour_idx, tour_logp, nodes, reward = actor(_Windows(), tour=tour, steppers=(rp, rp), record=True)
    assert rp.k == N and rp.handed_over
    assert np.array_equal(tour_idx.numpy(), z["tour_idx"]) and np.array_equal(nodes.numpy(), z["nodes"])
    assert tour_logp.dtype is torch.float64 and tuple(tour_logp.shape) == (B, N)
    assert len(actor.last_record) == N
    worst = dict(logits=0.0, last_hh=0.0)
    for k, rec in enumerate(actor.last_record):
        worst["logits"] = max(worst["logits"], float(np.abs(rec["logits"].numpy() - z["logits"][:, k]).max()))
        worst["last_hh"] = max(worst["last_hh"], float(np.abs(rec["last_hh"].numpy()[0] - z["last_hh"][:, k]).max()))
    err = float(np.abs(tour_logp.numpy() - z["tour_logp"]).max())
    print("float64 module against the reference: logits %.3g last_hh %.3g tour_logp %.3g" % (worst["logits"], worst["last_hh"], err))
    assert worst["logits"] <= 1e-10 and worst["last_hh"] <= 1e-10 and err <= 1e-10
    assert np.array_equal(reward.numpy(), -z["ratio"])
    assert not torch.is_grad_enabled() or not tour_logp.requires_grad        # the whole body runs under no_grad


def test_with_rows():
    actor = _actor().eval()
    window = torch.arange(3 * 3 * 20, dtype=torch.float32).reshape(3, 3, 20)
    base = actor.pointer.fold_static(actor.static_encoder, window[:, 1:, :])
    assert base.xs.is_contiguous()
    sf = base.with_rows(window[:, 1:, :])
    assert sf.xs.data_ptr() == window[:, 1:, :].data_ptr() and not sf.xs.is_contiguous()
    assert sf.G is base.G and sf.g is base.g and sf.static_encoder is base.static_encoder and (sf.nR, sf.S) == (20, 2)
    assert rollout._rows_view_stride(sf.xs) == 60 and rollout._rows_view_stride(base.xs) == 40
    wide = torch.zeros(3, 5, 20)
    for bad in (wide[:, ::2, :][:, :2],                      # rows 40 apart
                torch.zeros(3, 2, 40)[:, :, ::2],            # the last axis strided
                torch.zeros(3, 20, 2).transpose(1, 2),       # transposed rows
                torch.zeros(3, 3, 20), torch.zeros(3, 2, 24), torch.zeros(2, 20), torch.zeros(3, 2, 20, dtype=torch.int64)):
        with pytest.raises(ValueError):
            base.with_rows(bad)
    one = base.with_rows(torch.zeros(1, 2, 20))             # a single env has no env stride to check
    assert rollout._rows_view_stride(one.xs) == 40


def test_entry_checks_need_no_device():
    """tap_pointer_pick_static's argument checks in the header's order, with a null context and host addresses that are never
    dereferenced"""
    L = _lib.lib()
    assert "tap_pointer_pick_static" in _lib.EXPORTS and hasattr(L, "tap_pointer_pick_static")
    assert (_lib.TAP_PICK_GREEDY, _lib.TAP_PICK_DRAW) == (1, 2)
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    off = C.c_void_p(p.value + 4)
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED
    names = ("xs", "bits", "G", "g", "M", "k", "q", "va", "vp", "mask", "ptr", "logp")

    def f(B=1, nR=20, rows=30, Hd=64, S=2, stride=40, form=1, state=None, logits=None, **over):
        a = dict.fromkeys(names, p)
        a.update(over)
        return L.tap_pointer_pick_static(None, a["xs"], stride, a["bits"], B, nR, rows, Hd, S, a["G"], a["g"], a["M"], a["k"], a["q"],
                                         a["va"], a["vp"], a["mask"], form, state, 0, 0, a["ptr"], a["logp"], logits, None)
    # 1. dimensions and the form, before anything else
    for bad in (dict(B=-1), dict(nR=0), dict(rows=0), dict(Hd=0), dict(S=0), dict(form=0), dict(form=3)):
        assert f(**bad) == inv, bad
        assert f(xs=None, **bad) == inv
    # 2. an empty batch is fine whatever the buffers and the shape are
    assert f(B=0, xs=None, mask=None) == ok and f(B=0, Hd=96) == ok
    # 3. null buffers, before the state, the stride and the shape are looked at; logits_out may be null
    for hole in names:
        assert f(**{hole: None}) == inv and f(Hd=96, **{hole: None}) == inv, hole
    # 4. DRAW's state; greedy does not look at it
    assert f(form=2) == inv and f(form=2, state=off) == inv and f(form=2, state=off, Hd=96) == inv
    assert f(form=2, state=p, Hd=96) == uns and f(form=1, state=off, Hd=96) == uns
    # 5. the env stride of xs, before the shape
    assert f(stride=39) == inv and f(stride=39, Hd=96) == inv and f(stride=40, Hd=96) == uns and f(stride=60, Hd=96) == uns
    # 6. the shapes without a kernel
    for bad in (dict(Hd=96), dict(nR=6, stride=12), dict(rows=129), dict(S=9, stride=180), dict(nR=260, stride=520)):
        assert f(**bad) == uns, bad
    # 7. the alignment: bits and ptr_out 8 bytes, floats 4
    half = C.c_void_p(p.value + 2)
    assert f(ptr=off) == inv and f(bits=off) == inv and f(xs=half) == inv and f(logp=half) == inv and f(logits=half) == inv
    # the geometry entry describes this launch too: the static-rows form's, no LDS of its own
    assert _lib.pointer_scores_geometry(3074, 20, 30, 128, 2)[0] == 3 and _lib.pointer_scores_geometry(5123, 4, 10, 64, 2)[0] == 5


def test_wrapper_checks_run_before_the_device():
    z = lambda *s: torch.zeros(*s)                                                       # noqa: E731
    Hd, S, nR, rows, Bn = 64, 2, 20, 30, 3
    good = dict(xs=z(Bn, S, nR), bits=z(Bn, nR).long(), G=z(3 * Hd, S), g=z(3 * Hd), M=z(3 * Hd, rows), k=z(3 * Hd), q=z(Bn, Hd),
                va=z(Hd), vp=z(Hd), mask=z(Bn, nR))
    order = ("xs", "bits", "G", "g", "M", "k", "q", "va", "vp", "mask")
    for name, bad in (("xs", z(Bn, 9, nR)), ("G", z(3 * Hd, S + 1)), ("q", z(Bn + 1, Hd)), ("mask", z(Bn, nR + 1)), ("mask", z(Bn, nR).long()),
                      ("M", z(3 * 96, rows)), ("bits", z(Bn, nR + 4).long())):
        args = dict(good)
        args[name] = bad
        with pytest.raises(ValueError):
            T.pointer_pick_static(*(args[n] for n in order))
    with pytest.raises(TypeError):
        T.pointer_pick_static(*(dict(good, bits=z(Bn, nR))[n] for n in order))
    with pytest.raises(ValueError, match="no backward"):
        T.pointer_pick_static(*(dict(good, G=z(3 * Hd, S).requires_grad_(True))[n] for n in order))
    with pytest.raises(ValueError):                                                      # a pick record with a bad state
        T.pointer_pick_static(*(good[n] for n in order), source=(z(2), 0))
    with pytest.raises(T.TapError):                                                      # well-formed arguments on the host: no CPU path
        T.pointer_pick_static(*(good[n] for n in order))
