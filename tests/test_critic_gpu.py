"""The state critic on the bit shadow on the MI355X (critic.hip: k_critic_value<HPL>, k_critic_value_bw<HPL>,
k_critic_value_bw_reduce) against the float64 model of tests/critic_model.py and the reference's recorded critic
(tests/golden/critic_*.npz).

The tolerance is not a constant.  Per case the reference's own form (a Conv1d over the fp32 dynamic, then per block a
concatenation, a bmm, a softmax and a context bmm -- trainer.py:18-94) is evaluated in float32 torch on the CPU; its
largest error against float64 is ``e_ref``, and the kernel must stay within 4 e_ref + 16 * 2^-24 * max |want|
(pointer_model.tolerance).  The kernel's inputs are the float64 fold of the case rounded to float32, and `want` is the
float64 model ON those rounded inputs, so no input rounding enters the comparison.  Each test prints its worst err / e_ref."""
import numpy as np
import pytest
import torch

import critic_model as M
import golden_util
import tap_net_amd as T
from tap_net_amd import _lib, rollout, tools

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (rows, nR, H, S, n, B): one and two shadow planes; H 64 / 128 / 256 = 1, 2 and 4 hidden rows per lane; nR below and above
# 64 (the softmax then takes several columns per lane); U resident in LDS and recomputed per block, for each M staged whole
# and by 64-row slabs; n = 1 and n > 1; S = 2, 3 and 4; B = 1; four envs per workgroup: a last workgroup that is full (B = 4)
# and ragged ones
CASES = [(10, 4, 64, 2, 1, 1), (30, 20, 128, 2, 3, 67), (30, 60, 128, 3, 3, 3), (63, 68, 64, 4, 2, 4), (65, 20, 128, 3, 3, 3),
         (126, 60, 256, 3, 3, 2), (128, 256, 64, 2, 3, 3), (10, 8, 256, 2, 2, 5)]
DENSITIES = (0.0, 0.1, 1.0)
BW_CASES = [(30, 20, 128, 2, 3, 67, True), (65, 20, 128, 3, 3, 3, False), (126, 60, 256, 3, 3, 2, False), (63, 68, 64, 4, 2, 4, False)]
FIXTURES = ["critic_%dd_%s.npz" % (D, ws) for D in (2, 3) for ws in ("xavier", "sharp")]


def _geom(rows, nR, H, backward):
    """(U / dU resident, hidden rows per lane, shadow planes, M staged whole) the launcher picks: a 64 KB LDS budget for M (whole
    up to 32 KB, else one 64-row slab), nR floats per wavefront, the backward's dv partials and the four envs' U"""
    mall = 1 if H == 64 or rows * (H + 1) * 4 <= 32 * 1024 else 0
    base = rows * ((H if mall else 64) + 1) + 4 * nR + (4 * H if backward else 0)
    return (1 if (base + 4 * nR * (H + 1)) * 4 <= 64 * 1024 else 0, H // 64, M.planes_of(rows), mall)


def _key(rows, nR, H, backward):
    res, hpl, planes, mall = _geom(rows, nR, H, backward)
    return (_lib.TAP_HIT_CRITIC, res, hpl, planes, mall, 1 if backward else 0, 0)


def _keys(extra):
    return {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_CRITIC and k[5] == extra}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _inputs(rows, nR, H, S, n, B, density, seed):
    """-> X (the reference form's inputs), the kernel's float32 inputs (x, G, g, M, q0, v, w2, b2), the shadow"""
    X = M.make_case(B, rows, nR, H, S, n, density, seed)
    G, g, Mf, q0 = (np.asarray(a, np.float32) for a in M.fold(X, np.float64))
    return X, (X["x"], G, g, Mf, q0, X["v"], X["w2"], X["b2"]), M.pack_bits(X["dyn"])


def _raw(inp, bits, rows, n):
    """the forward entry on device copies -> value, z, p, xbar as numpy"""
    x, G, g, Mf, q0 = inp[:5]
    B, S, nR = x.shape
    H = Mf.shape[0]
    out = [torch.full(s, float('nan'), device=DEV) for s in ((B,), (B, H), (B, n, nR), (B, n, S), (B, n, H))]
    rollout._critic_into(_dev(inp[0]), _dev(bits), *(_dev(a) for a in inp[1:]), n, rows, *out)
    assert np.array_equal(out[4][:, 0].cpu().numpy(), np.broadcast_to(q0, (B, H)))      # q[:, 0] = q0
    return [o.cpu().numpy() for o in out[:4]] + [out[4].cpu().numpy()]


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))


def _e_ref(X):
    with torch.no_grad():
        r32, r64 = M.reference_form_torch(X, torch.float32), M.reference_form_torch(X, torch.float64)
    return [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)]


def test_case_list_covers_every_axis():
    """from the launch record of one call per case (zero inputs: only the geometry matters)"""
    seen = set()
    for rows, nR, H, S, n, B in CASES:
        _lib.variant_hits_reset(DEV)
        z = lambda *s: torch.zeros(*s, device=DEV)
        bits = torch.zeros(B, M.planes_of(rows) * nR, dtype=torch.int64, device=DEV)
        with torch.no_grad():
            out = T.critic_value(z(B, S, nR), bits, z(3 * H, S), z(3 * H), z(H, rows), z(B, H), z(H), z(H), z(1), n)
        assert tuple(out.shape) == (B,) and not bool(out.any())
        keys = _keys(0)
        assert keys == {_key(rows, nR, H, False)}, keys
        seen |= keys
    assert {k[3] for k in seen} == {1, 2}                                          # both shadow planes
    assert {k[2] for k in seen} == {1, 2, 4}                                       # every instantiation the launcher can pick
    assert {(k[1], k[4]) for k in seen} == {(0, 0), (0, 1), (1, 0), (1, 1)}        # U resident / recomputed x M whole / by slabs
    assert {(k[1], k[2]) for k in seen} >= {(1, 1), (1, 2), (1, 4), (0, 1), (0, 2), (0, 4)}
    assert {_key(*c[:3], True)[1:5] for c in BW_CASES} == {(1, 2, 1, 1), (1, 2, 2, 0), (0, 4, 2, 0), (0, 1, 1, 1)}
    assert min(c[1] for c in CASES) < 64 < max(c[1] for c in CASES) and {c[1] for c in CASES} >= {4, 20, 60, 68, 256}
    assert {c[3] for c in CASES} >= {2, 4} and {c[4] for c in CASES} >= {1, 3} and any(c[5] == 1 for c in CASES)
    assert any(c[5] % 4 == 0 for c in CASES) and any(c[5] > 4 and c[5] % 4 for c in CASES)    # a full and a ragged last workgroup


@pytest.mark.parametrize("rows,nR,H,S,n,B", CASES)
def test_forward(rows, nR, H, S, n, B):
    worst = 0.0
    for i, density in enumerate(DENSITIES):
        X, inp, bits = _inputs(rows, nR, H, S, n, B, density, 1000 * rows + 10 * nR + i)
        with torch.no_grad():
            want = [w.numpy() for w in M.folded_torch(_t(inp[0]), _t(X["dyn"]), *(_t(a) for a in inp[1:]), n)]
        e_ref = _e_ref(X)
        _lib.variant_hits_reset(DEV)
        got = _raw(inp, bits, rows, n)
        assert _keys(0) == {_key(rows, nR, H, False)}
        for name, g, w, e in zip(M.NAMES, got, want, e_ref):
            assert g.dtype == np.float32 and g.shape == w.shape and np.isfinite(g).all(), name
            err = float(np.abs(g.astype(np.float64) - w).max())
            print("critic forward %s density %.1f %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
                  % ((rows, nR, H, S, n, B), density, name, err, e, _ratio(err, e), np.abs(w).max()))
            assert err <= M.tolerance(e, w), (name, density, err, e)
            worst = max(worst, _ratio(err, e))
        assert abs(got[2].sum(2) - 1).max() <= 1e-5                                # p is a softmax over ALL columns
        # two calls give the same bytes; garbage above `rows` changes no byte
        again = _raw(inp, bits, rows, n)
        junk = _raw(inp, M.garbage(bits, rows, nR, 7), rows, n)
        for a, b, c in zip(got, again, junk):
            assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes()
        if density == 0.0:
            # an all-zero shadow: M does not enter, whatever it holds
            other = _raw(inp[:3] + (np.full_like(inp[3], 1e30),) + inp[4:], bits, rows, n)
            for a, b in zip(got, other):
                assert a.tobytes() == b.tobytes()
        if density == 0.1:
            # one q0 row for the whole batch (stride 0) = that row expanded
            one = inp[:4] + (inp[4][:1],) + inp[5:]
            wide = inp[:4] + (np.ascontiguousarray(np.broadcast_to(inp[4][:1], inp[4].shape)),) + inp[5:]
            for a, b in zip(_raw(one, bits, rows, n), _raw(wide, bits, rows, n)):
                assert a.tobytes() == b.tobytes()
    print("critic forward %s: worst err / e_ref %.2f" % ((rows, nR, H, S, n, B), worst))


GRADS = ("dG", "dg", "dM", "dq0", "dv", "dw2", "db2")


def _grads_torch(inp, dyn, a, n, dtype):
    """autograd of the folded model in torch on the CPU -> dG, dg, dM, dq0, dv, dw2, db2"""
    leaves = [_t(v, dtype).requires_grad_(True) for v in inp[1:]]
    value = M.folded_torch(_t(inp[0], dtype), _t(dyn, dtype), *leaves, n)[0]
    (value * _t(a, dtype)).sum().backward()
    return [v.grad.double().numpy() for v in leaves]


def _grads_device(inp, bits, a, rows, n):
    leaves = [_dev(v).requires_grad_(True) for v in inp[1:]]
    mine = _dev(bits)
    value = T.critic_value(_dev(inp[0]), mine, *leaves, n, rows=rows)
    assert value.requires_grad
    mine.fill_(-1)                                                                 # the caller's shadow is overwritten before the backward
    value.backward(_dev(a))
    return [v.grad.cpu().numpy() for v in leaves]


@pytest.mark.parametrize("rows,nR,H,S,n,B,bcast", BW_CASES)
def test_backward(rows, nR, H, S, n, B, bcast):
    X, inp, bits = _inputs(rows, nR, H, S, n, B, 0.1, 77 * rows + nR)
    if bcast:
        inp = inp[:4] + (inp[4][:1],) + inp[5:]                                    # q0 (1, H): dq0 is the sum over the batch
    a = np.random.RandomState(rows + B).randn(B).astype(np.float32)
    want = _grads_torch(inp, X["dyn"], a, n, torch.float64)
    ref32 = _grads_torch(inp, X["dyn"], a, n, torch.float32)
    _lib.variant_hits_reset(DEV)
    got = _grads_device(inp, bits, a, rows, n)
    assert _keys(1) == {_key(rows, nR, H, True)} and _keys(0) == {_key(rows, nR, H, False)}
    worst = 0.0
    for name, g, w, r in zip(GRADS, got, want, ref32):
        assert g.dtype == np.float32 and g.shape == w.shape and np.isfinite(g).all(), name
        e = float(np.abs(r - w).max())
        err = float(np.abs(g.astype(np.float64) - w).max())
        print("critic backward %s %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
              % ((rows, nR, H, S, n, B), name, err, e, _ratio(err, e), np.abs(w).max()))
        assert np.abs(w).max() > 0 and err <= M.tolerance(e, w), (name, err, e)
        worst = max(worst, _ratio(err, e))
    print("critic backward %s: worst err / e_ref %.2f" % ((rows, nR, H, S, n, B), worst))
    again = _grads_device(inp, bits, a, rows, n)                                   # deterministic: the same bytes
    for g, b in zip(got, again):
        assert g.tobytes() == b.tobytes()


def _fixture(name):
    z = golden_util.load(name)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")}
    D = int(z["static_input"].shape[1])
    net = tools.StateCritic(D, int(z["dynamic"].shape[1]), int(sd["attention.v"].shape[2]), n_process_blocks=int(z["p"].shape[1]))
    net.load_state_dict(sd, strict=True)
    return z, D, net


@pytest.mark.parametrize("name", FIXTURES)
def test_module_on_the_shadow_equals_the_recorded_reference(name):
    """StateCritic.forward on pack.dynamic_bits of the recorded dynamic, in training mode (drop_hh does not reach the
    estimate): the estimates and all 16 gradients within 4 e_ref + 16 ulp, the fixture's own e_ref; one critic launch
    forward and one backward pair; the stepper's shadow before step 0 gives the same bytes"""
    z, D, net = _fixture(name)
    net = net.to(DEV).train()
    x = _dev(z["static_input"].astype(np.float32))
    dynamic = _dev(z["dynamic"].astype(np.float32))
    bits, nonbinary = T.pack.dynamic_bits(dynamic)
    assert bits.dtype is torch.int64 and int(nonbinary) == 0
    _lib.variant_hits_reset(DEV)
    est = net(x, bits)
    assert tuple(est.shape) == (x.shape[0], 1)
    (est.view(-1) * _dev(z["a"].astype(np.float32))).sum().backward()
    hits = {extra: sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == _lib.TAP_HIT_CRITIC and k[5] == extra) for extra in (0, 1)}
    assert hits == {0: 1, 1: 1}, hits
    got = est.detach().view(-1).double().cpu().numpy()
    err, e = float(np.abs(got - z["est"]).max()), float(z["e_ref_est"])
    print("%s est: err %.3g e_ref %.3g ratio %.2f" % (name, err, e, _ratio(err, e)))
    assert err <= M.tolerance(e, z["est"])
    grads = dict(net.named_parameters())
    assert len(grads) == 16
    for k, p in sorted(grads.items()):
        w, e = z["grad_" + k], float(z["e_ref_grad_" + k])
        err = float(np.abs(p.grad.double().cpu().numpy() - w).max())
        print("%s grad %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g" % (name, k, err, e, _ratio(err, e), np.abs(w).max()))
        assert err <= M.tolerance(e, w), (k, err, e)
    # the stepper's own shadow, taken before step 0
    n_blocks = 10
    ds = golden_util.load("dataset_%dd.npz" % D)
    B = int(x.shape[0])
    static = _dev(ds["static"][:B].astype(np.float32))
    assert np.array_equal(ds["dynamic"][:B], z["dynamic"]) and np.array_equal(ds["static"][:B, 1:1 + D], z["static_input"])
    env = T.BatchedContainer(B, [5] * (D - 1) + [50], n_blocks, "C+P+S-lb-soft", "diff", device=DEV)
    with torch.no_grad():
        sp = T.EpisodeStepper(static, dynamic, env, expand_dynamic=False).begin(static, dynamic)
        assert torch.equal(net(x, sp.dynamic_bits), net(x, bits)) and torch.equal(net(x, bits), est.detach())


def test_forward_replays_from_a_hip_graph():
    z, D, net = _fixture(FIXTURES[1])
    net = net.to(DEV).eval()
    x = _dev(z["static_input"].astype(np.float32))
    bits = T.pack.dynamic_bits(_dev(z["dynamic"].astype(np.float32)))[0]
    with torch.no_grad():
        eager = net(x, bits)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            net(x, bits)
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = net(x, bits)
        for _ in range(2):
            rec.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(rec, eager)
    assert bool(torch.isfinite(eager).all()) and float(eager.abs().max()) > 0
