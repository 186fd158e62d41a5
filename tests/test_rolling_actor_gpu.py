"""tools.RollingDRL on the MI355X.

Against the reference: tests/golden/rolling_actor_2d.npz (rolling.DRL in rolling.validate's loop), the state dict loaded
strictly, eval(), teacher-forced on the recorded tour on the REAL steppers (RollingStepper, then the last graph's
EpisodeStepper): per-step ``logits`` and ``last_hh`` under pointer_model.tolerance with the fixture's own e_ref; ``nodes``, the
five validate figures and the reward exact.  Against the two-launch composition: free-running eval() with ``fused_pick`` on and
off gives the same bytes of all four outputs (2D and 3D), and so does train() (DRAW, dropout 0.1), where two modules of one
seed draw the same tours.  One eval call replays from a graph with the eager bytes.  ``rolling.validate`` writes the
reference's six files."""
import os

import numpy as np
import pytest
import torch

import pointer_model as PM
import tap_net_amd as T
from tap_net_amd import _lib, pack
from tap_net_amd import generate as gen
from tap_net_amd import rolling as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rolling_actor_2d.npz")
HE, HD, CHILD = 32, 64, 10
REWARD = "C+P+S-lb-soft"
FREE = {2: (67, 14, [7, 100], 70), 3: (35, 12, [7, 7, 100], 70)}      # D: B, N, initial container, target height


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits32(t):
    return t.view(torch.int32) if t.dtype is torch.float32 else t


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits32(a), _bits32(b))


def _actor(D, height, z=None, dropout=0.1, **kw):
    actor = T.RollingDRL(D, 3 * CHILD, HE, HD, True, 'bot', True, 5, height, D, REWARD, 'shape_heightmap', "diff", "LB_GREEDY",
                         None, pack.update_dynamic, pack.update_mask, 1, dropout, 1, **kw)
    if z is not None:
        actor.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")}, strict=True)
    return actor.to(DEV)


def _fixture_windows(z):
    return T.RollingWindows(_dev(z["blocks"].astype(np.int32)), _dev(z["positions"].astype(np.int32)),
                            [int(v) for v in z["initial_container_size"]], child_graph_size=CHILD)


class _Data(object):
    def __init__(self, windows):
        self.windows = windows


_FORCED = {}


def _forced():
    """the module teacher-forced on the fixture's tour through rolling.validate, made once and left unchanged"""
    if not _FORCED:
        z = np.load(GOLDEN)
        actor = _actor(2, int(z["container_size"][1]), z).eval()
        _lib.variant_hits_reset(DEV)
        figures = R.validate(actor, _Data(_fixture_windows(z)), tour=_dev(z["tour_idx"].astype(np.int64)))
        torch.cuda.synchronize()
        hits = _lib.variant_hits(DEV)
        # validate's own call keeps no record: a second forced call does (record=True keeps the logits)
        out = actor(_fixture_windows(z), tour=_dev(z["tour_idx"].astype(np.int64)), record=True)
        actor.last_stepper.check()
        _FORCED.update(z=z, figures=figures, hits=hits, out=[t.cpu().numpy() for t in out],
                       logits=np.stack([r["logits"].cpu().numpy() for r in actor.last_record], 1).astype(np.float64),
                       last_hh=np.stack([r["last_hh"][0].cpu().numpy() for r in actor.last_record], 1).astype(np.float64))
    return _FORCED


def test_fixture_teacher_forced_on_the_real_steppers():
    f = _forced()
    z = f["z"]
    N = z["tour_idx"].shape[1]
    failed, worst = [], 0.0
    for name in ("logits", "last_hh"):
        for k in range(N):
            want, got, e = z[name][:, k], f[name][:, k], float(z["e_ref_" + name][k])
            err, tol = float(np.abs(got - want).max()), PM.tolerance(e, want)
            worst = max(worst, err / max(e, 1e-30))
            print("rolling actor %s step %d: err %.3g e_ref %.3g tolerance %.3g max|want| %.3g" % (name, k, err, e, tol, np.abs(want).max()))
            if not (np.isfinite(got).all() and err <= tol):
                failed.append((name, k, err, tol))
    print("rolling actor: worst err / e_ref %.2f" % worst)
    assert not failed, failed
    tour_idx, tour_logp, nodes, reward = f["out"]
    assert np.array_equal(tour_idx, z["tour_idx"]) and np.array_equal(nodes, z["nodes"])
    err = float(np.abs(tour_logp.astype(np.float64) - z["tour_logp"]).max())
    tol = PM.tolerance(float(z["e_ref_tour_logp"]) + 2 * float(z["e_ref_logits"].max()), z["tour_logp"])
    print("rolling actor tour_logp: err %.3g tolerance %.3g" % (err, tol))
    assert err <= tol
    assert np.array_equal(reward, (-z["ratio"]).astype(np.float32))
    for got, want in zip(f["figures"], z["metrics"].T):
        assert got.dtype == np.float64 and np.array_equal(got, want)
    # the teacher-forced call is the two-launch path: N static-rows launches and N of the head's GIVEN form, none fused
    ptr_hits = {k: v for k, v in f["hits"].items() if k[0] == _lib.TAP_HIT_POINTER}
    assert sum(ptr_hits.values()) == N and all(k[1] == 0 and k[6] == 2 for k in ptr_hits)
    assert sum(v for k, v in f["hits"].items() if k[0] == _lib.TAP_HIT_POLICY_PICK and k[3] == 3) == N


def test_validate_writes_the_references_files(tmp_path):
    z = np.load(GOLDEN)
    actor = _actor(2, int(z["container_size"][1]), z)
    out = R.validate(actor, _Data(_fixture_windows(z)), str(tmp_path / "render"), tour=_dev(z["tour_idx"].astype(np.int64)))
    assert not actor.training
    names = sorted(os.listdir(str(tmp_path / "render")))
    assert names == sorted("batch-%s.txt" % n for n in ("valid_size", "box_size", "empty_size", "stable_num", "packing_height", "time"))
    for k, name in enumerate(("valid_size", "box_size", "empty_size", "stable_num", "packing_height")):
        got = np.loadtxt(str(tmp_path / "render" / ("batch-%s.txt" % name)))
        assert np.array_equal(got, z["metrics"][:, k]) and np.array_equal(out[k], z["metrics"][:, k]), name
    t = np.loadtxt(str(tmp_path / "render" / "batch-time.txt"))
    assert t.shape == (z["metrics"].shape[0],) and (t > 0).all() and (t == t[0]).all()
    # free-running (the reference's call): the same figures wherever float32 picks the float64 tour, and always well-formed
    free = R.validate(actor, _Data(_fixture_windows(z)))
    assert all(a.shape == (5,) and np.isfinite(a).all() for a in free) and not free[4].any()


def _instances(D):
    B, N, init, H = FREE[D]
    _, _, blocks, positions = gen.generate_instances(B, N, D, init[0], init[-1], 1, (1, 5), seed=11 + D, device=DEV, return_aux=True)
    return blocks, positions, init, N, H


def _hits(kind):
    return {k: v for k, v in _lib.variant_hits(DEV).items() if k[0] == kind}


@pytest.mark.parametrize("D", [2, 3])
def test_eval_fused_and_unfused_give_the_same_bytes(D):
    blocks, positions, init, N, H = _instances(D)
    torch.manual_seed(40 + D)
    on = _actor(D, H).eval()
    off = _actor(D, H, fused_pick=False).eval()
    off.load_state_dict(on.state_dict(), strict=True)
    _lib.variant_hits_reset(DEV)
    got = on(T.RollingWindows(blocks, positions, init, CHILD))
    torch.cuda.synchronize()
    ptr_hits, head_hits = _hits(_lib.TAP_HIT_POINTER), _hits(_lib.TAP_HIT_POLICY_PICK)
    assert sum(ptr_hits.values()) == N and all(k[1] == 1 for k in ptr_hits) and not head_hits      # N fused greedy launches, no head
    _lib.variant_hits_reset(DEV)
    want = off(T.RollingWindows(blocks, positions, init, CHILD))
    torch.cuda.synchronize()
    ptr_hits, head_hits = _hits(_lib.TAP_HIT_POINTER), _hits(_lib.TAP_HIT_POLICY_PICK)
    assert sum(ptr_hits.values()) == N and all(k[1] == 0 for k in ptr_hits) and sum(head_hits.values()) == N
    for a, b in zip(got, want):
        assert _same(a, b)
    tour_idx, tour_logp, nodes, reward = got
    assert tour_idx.dtype is torch.int64 and tour_logp.dtype is torch.float32 and nodes.dtype is torch.int32
    assert tuple(tour_idx.shape) == tuple(tour_logp.shape) == tuple(nodes.shape) == (FREE[D][0], N)
    assert bool(torch.isfinite(tour_logp).all()) and bool(torch.isfinite(reward).all())
    assert torch.equal(nodes.long().sort(1).values, torch.arange(N, device=DEV).expand_as(nodes))
    on.last_stepper.check()
    # record=True keeps the bytes and each step's logits
    again = on(T.RollingWindows(blocks, positions, init, CHILD), record=True)
    for a, b in zip(again, want):
        assert _same(a, b)
    assert len(on.last_record) == N and tuple(on.last_record[0]["logits"].shape) == (FREE[D][0], CHILD * (2 if D == 2 else 6))


class _Watch(object):
    """a stepper handed through, keeping whether every pick was selectable under the mask it was made with"""

    def __init__(self, sp, seen):
        self.__dict__.update(_sp=sp, _seen=seen)

    def __getattr__(self, name):
        return getattr(self._sp, name)

    def __setattr__(self, name, value):
        setattr(self._sp, name, value)

    def step(self, ptr):
        self._seen.append(bool((self._sp.current_mask.gather(1, ptr.unsqueeze(1)) != 0).all()))
        return self._sp.step(ptr)


def test_train_draws_the_same_tours_fused_and_unfused():
    D = 2
    blocks, positions, init, N, H = _instances(D)
    torch.manual_seed(50)
    a = _actor(D, H, seed=77).train()
    b = _actor(D, H, seed=77).train()
    c = _actor(D, H, seed=77, fused_pick=False).train()
    for m in (b, c):
        m.load_state_dict(a.state_dict(), strict=True)
    seen = []
    pair = a._own_pair(T.RollingWindows(blocks, positions, init, CHILD))
    watched = (_Watch(pair[0], seen), _Watch(pair[1], seen))
    tours = []
    for episode in (1, 2):
        outs = [a(T.RollingWindows(blocks, positions, init, CHILD), steppers=watched),
                b(T.RollingWindows(blocks, positions, init, CHILD)),
                c(T.RollingWindows(blocks, positions, init, CHILD))]
        for other in outs[1:]:
            for x, y in zip(outs[0], other):
                assert _same(x, y), episode
        tour_idx, tour_logp, nodes, reward = outs[0]
        assert a.step_dropout(DEV).state.tolist() == [77, episode]
        assert torch.equal(nodes.long().sort(1).values, torch.arange(N, device=DEV).expand_as(nodes))
        assert not bool(torch.isnan(reward).any()) and bool(torch.isfinite(tour_logp).all())
        tours.append(tour_idx.clone())
    assert seen == [True] * (2 * N) and not torch.equal(tours[0], tours[1])
    a.last_stepper.check()


def test_eval_call_replays_from_a_graph():
    """one eval call at the 2D shape captured under pack.set_binary_check('trust') -- the windows' state restored at its head,
    as a caller that replays must -- and replayed twice: the eager bytes"""
    D = 2
    blocks, positions, init, N, H = _instances(D)
    torch.manual_seed(60)
    actor = _actor(D, H).eval()
    rw = T.RollingWindows(blocks, positions, init, CHILD)
    state0 = rw.state.clone()

    def call():
        rw.state.copy_(state0)
        rw.steps_done = 0
        return actor(rw)
    pack.set_binary_check('trust')
    try:
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            want = [t.clone() for t in call()]
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = call()
        torch.cuda.synchronize()
        for _ in range(2):
            for t in rec:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(rec, want):
                assert _same(a, b)
    finally:
        pack.set_binary_check('check')
