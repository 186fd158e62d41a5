"""The pointer network on the bit shadow on the MI355X (pointer.hip: k_pointer_scores<HPL>, k_pointer_scores_bw<HPL>,
k_pointer_scores_bw_reduce) against the float64 model of tests/pointer_model.py.

The tolerance is not a constant.  Per case the reference's own form (two concatenations, two bmm, a softmax, a context
bmm -- model.py:38-138) is evaluated in float32 torch on the CPU; its largest error against float64 is ``e_ref``, and the
kernel must stay within 4 e_ref + 16 * 2^-24 * max |want| (pointer_model.tolerance: the factor covers the device's tanhf /
expf being a few ulp off and another order of the sums, the floor keeps a lucky e_ref from failing a correct kernel).
The kernel's inputs are the float64 fold of the case rounded to float32, and `want` is the float64 model ON those
rounded inputs, so no input rounding enters the comparison.  Each test prints its worst err / e_ref."""
import copy

import numpy as np
import pytest
import torch

import pointer_model as M
import tap_net_amd as T
from tap_net_amd import _lib, rollout, synth, tools

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (rows, nR, Hd, B): one and two shadow planes; Hd 64 / 128 / 256; one and two hidden rows per lane (two: one plane and
# Hd > 64) with 1, 2 and 4 hidden chunks per segment; nR below and above 64 (a wavefront's softmax then takes several
# columns per lane); batches of one env per workgroup and -- B >= 2048 -- of two, with a full (2050) and a ragged (2051)
# last workgroup
CASES = [(10, 4, 64, 1), (30, 20, 128, 67), (30, 60, 128, 3), (63, 68, 64, 3), (65, 20, 128, 3), (126, 60, 256, 2),
         (128, 256, 64, 3), (30, 20, 128, 2050), (10, 4, 64, 2051)]
DENSITIES = (0.0, 0.1, 1.0)
BW_CASES = [(30, 20, 128, 67), (65, 68, 64, 3), (126, 60, 256, 2), (10, 4, 64, 2050), (10, 4, 64, 2051)]


def _geom(rows, Hd):
    """(hidden rows per lane, shadow planes, hidden chunks per segment) the launcher picks"""
    planes = M.planes_of(rows)
    hpl = 2 if planes == 1 and Hd > 64 else 1
    return hpl, planes, Hd // (64 * hpl)


def _epb(B):
    return max(1, B // 1024)            # envs per workgroup (every case's LDS fits the budget at this count)


def _keys(extra):
    return {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_POINTER and k[5] == extra}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _inputs(rows, nR, Hd, B, density, seed):
    """-> X (the reference form's inputs), the kernel's float32 inputs (proj in the contract's natural order), the shadow"""
    X = M.make_case(B, rows, nR, Hd, Hd, density, seed)
    proj, Mf, k, q = (np.asarray(a, np.float32) for a in M.fold(X, np.float64))
    return X, (proj, Mf, k, q, X["va"], X["vp"]), M.pack_bits(X["dyn"])


def _raw(inp, bits, rows):
    """the forward entry on device copies -> logits, attn, t as numpy"""
    proj, Mf, k, q, va, vp = inp
    B, H3, nR = proj.shape
    Hd = H3 // 3
    out = [torch.full(s, float('nan'), device=DEV) for s in ((B, nR), (B, nR), (B, Hd))]
    rollout._scores_into(_dev(M.to_layout(proj)), _dev(bits), _dev(Mf), _dev(k), _dev(q), _dev(va), _dev(vp), rows, *out)
    return [o.cpu().numpy() for o in out]


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))


def _e_ref(X):
    with torch.no_grad():
        r32, r64 = M.reference_form_torch(X, torch.float32), M.reference_form_torch(X, torch.float64)
    return [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)]


def test_case_list_covers_every_axis():
    """from the launch record of one call per case (zero inputs: only the geometry matters)"""
    seen = set()
    for rows, nR, Hd, B in CASES:
        _lib.variant_hits_reset(DEV)
        z = lambda *s: torch.zeros(*s, device=DEV)
        bits = torch.zeros(B, M.planes_of(rows) * nR, dtype=torch.int64, device=DEV)
        with torch.no_grad():
            out = T.pointer_scores(z(B, 3, nR, Hd), bits, z(3 * Hd, rows), z(3 * Hd), z(B, Hd), z(Hd), z(Hd))
        assert tuple(out.shape) == (B, nR) and not bool(out.any())
        keys = _keys(0)
        assert keys == {(_lib.TAP_HIT_POINTER, 0) + _geom(rows, Hd) + (0, 0)}, keys
        seen |= keys
    assert {k[3] for k in seen} == {1, 2}                                          # both shadow planes
    assert {(k[2], k[3]) for k in seen} == {(1, 1), (2, 1), (1, 2)}                # every instantiation the launcher can pick
    assert {k[4] for k in seen} == {1, 2, 4}                                       # one and several hidden chunks
    assert {c[2] for c in CASES} == {64, 128, 256}
    assert min(c[1] for c in CASES) < 64 < max(c[1] for c in CASES) and {c[1] for c in CASES} >= {4, 20, 60, 68, 256}
    assert any(_epb(c[3]) > 1 and c[3] % _epb(c[3]) for c in CASES)                # a ragged last workgroup
    assert any(_epb(c[3]) > 1 and c[3] % _epb(c[3]) == 0 for c in CASES) and any(_epb(c[3]) == 1 and c[3] > 1 for c in CASES)


@pytest.mark.parametrize("rows,nR,Hd,B", CASES)
def test_forward(rows, nR, Hd, B):
    worst = 0.0
    for i, density in enumerate(DENSITIES):
        X, inp, bits = _inputs(rows, nR, Hd, B, density, 1000 * rows + 10 * nR + i)
        with torch.no_grad():
            want = [w.numpy() for w in M.folded_torch(_t64(inp[0]), _t64(X["dyn"]), *(_t64(a) for a in inp[1:]))]
        e_ref = _e_ref(X)
        _lib.variant_hits_reset(DEV)
        got = _raw(inp, bits, rows)
        assert _keys(0) == {(_lib.TAP_HIT_POINTER, 0) + _geom(rows, Hd) + (0, 0)}
        for name, g, w, e in zip(("logits", "attn", "t"), got, want, e_ref):
            assert g.dtype == np.float32 and g.shape == w.shape and np.isfinite(g).all()
            err = float(np.abs(g.astype(np.float64) - w).max())
            print("pointer forward %s density %.1f %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
                  % ((rows, nR, Hd, B), density, name, err, e, _ratio(err, e), np.abs(w).max()))
            assert err <= M.tolerance(e, w), (name, density, err, e)
            worst = max(worst, _ratio(err, e))
        assert abs(got[1].sum(1) - 1).max() <= 1e-5                                # attn is a softmax over ALL columns
        # two calls give the same bytes; garbage above `rows` changes no byte
        again = _raw(inp, bits, rows)
        junk = _raw(inp, M.garbage(bits, rows, nR, 7), rows)
        for a, b, c in zip(got, again, junk):
            assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes()
        if density == 0.0:
            # an all-zero shadow is the model with U = proj + k: M does not enter, whatever it holds
            other = _raw((inp[0], np.full_like(inp[1], 1e30)) + inp[2:], bits, rows)
            for a, b in zip(got, other):
                assert a.tobytes() == b.tobytes()
            proj, _, k, q, va, vp = inp
            with torch.no_grad():
                plain = M.folded_torch(_t64(proj), _t64(np.zeros_like(X["dyn"])), _t64(np.zeros_like(inp[1])), _t64(k), _t64(q),
                                       _t64(va), _t64(vp))
            assert float(np.abs(plain[0].numpy() - want[0]).max()) == 0.0
    print("pointer forward %s: worst err / e_ref %.2f" % ((rows, nR, Hd, B), worst))


def _grads_torch(inp, dyn, g, dtype):
    """autograd of the folded model in torch on the CPU -> dproj (natural order), dM, dk, dq, dva, dvp"""
    leaves = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in inp]
    logits = M.folded_torch(leaves[0], torch.from_numpy(dyn).to(dtype), *leaves[1:])[0]
    (logits * torch.from_numpy(g).to(dtype)).sum().backward()
    return [v.grad.double().numpy() for v in leaves]


def _grads_device(inp, bits, g, rows):
    proj, Mf, k, q, va, vp = inp
    leaves = [_dev(M.to_layout(proj))] + [_dev(a) for a in (Mf, k, q, va, vp)]
    for v in leaves:
        v.requires_grad_(True)
    mine = _dev(bits)
    logits = T.pointer_scores(leaves[0], mine, *leaves[1:], rows=rows)
    assert logits.requires_grad
    mine.fill_(-1)                                                                 # the caller's shadow is overwritten before the backward
    logits.backward(_dev(g))
    out = [v.grad.cpu().numpy() for v in leaves]
    out[0] = M.from_layout(out[0])
    return out


@pytest.mark.parametrize("rows,nR,Hd,B", BW_CASES)
def test_backward(rows, nR, Hd, B):
    X, inp, bits = _inputs(rows, nR, Hd, B, 0.1, 77 * rows + nR)
    g = np.random.RandomState(rows + B).randn(B, nR).astype(np.float32)
    want = _grads_torch(inp, X["dyn"], g, torch.float64)
    ref32 = _grads_torch(inp, X["dyn"], g, torch.float32)
    _lib.variant_hits_reset(DEV)
    got = _grads_device(inp, bits, g, rows)
    assert _keys(1) == {(_lib.TAP_HIT_POINTER, 0) + _geom(rows, Hd) + (1, 0)}
    worst = 0.0
    for name, a, w, r in zip(("dproj", "dM", "dk", "dq", "dva", "dvp"), got, want, ref32):
        assert a.dtype == np.float32 and a.shape == w.shape and np.isfinite(a).all(), name
        e = float(np.abs(r - w).max())
        err = float(np.abs(a.astype(np.float64) - w).max())
        print("pointer backward %s %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
              % ((rows, nR, Hd, B), name, err, e, _ratio(err, e), np.abs(w).max()))
        assert np.abs(w).max() > 0 and err <= M.tolerance(e, w), (name, err, e)
        worst = max(worst, _ratio(err, e))
    print("pointer backward %s: worst err / e_ref %.2f" % ((rows, nR, Hd, B), worst))
    again = _grads_device(inp, bits, g, rows)                                      # deterministic: the same bytes
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


def _xavier_(module):
    for p in module.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    return module


def _named_grads(net, enc, extra):
    out = {"pointer." + n: p.grad for n, p in net.named_parameters()}
    out.update({"encoder." + n: p.grad for n, p in enc.named_parameters()})
    out.update(extra)
    return {n: v.detach().double().cpu().numpy() for n, v in out.items()}


def test_forward_bits_gradients_through_the_modules():
    """tools.Pointer.forward_bits on the device against ``forward`` on the float path in float64 (and, for e_ref, in
    float32) on the CPU: the logits, last_hh and the gradient of every parameter, of conv.weight / conv.bias and of
    static_hidden.  The modules are in training mode with dropout 0.0: the GRU's device backward exists in training mode
    only, and without dropout that mode draws nothing"""
    B, rows, nR, H = 5, 30, 20, 128
    torch.manual_seed(31)
    net = _xavier_(tools.Pointer(H, H, 'shape_heightmap', 'bot', dropout=0.0)).train()
    enc = T.DynamicBitsEncoder(rows, H)
    rng = np.random.RandomState(32)
    dyn = rng.rand(B, rows, nR) < 0.1
    sh, dec, hh = torch.randn(B, H, nR), torch.randn(B, H, 1), torch.randn(1, B, H)
    g, ghh = torch.randn(B, nR), torch.randn(1, B, H)

    def float_path(dtype):
        n2, e2 = copy.deepcopy(net).to(dtype), copy.deepcopy(enc).to(dtype)
        s2 = sh.clone().to(dtype).requires_grad_(True)                 # (a clone: .to() of the same dtype is the tensor itself)
        logits, last = n2(s2, e2(torch.from_numpy(dyn).to(dtype)), dec.to(dtype), hh.to(dtype))
        ((logits * g.to(dtype)).sum() + (last * ghh.to(dtype)).sum()).backward()
        return logits.detach().double().numpy(), last.detach().double().numpy(), _named_grads(n2, e2, {"static_hidden": s2.grad})
    want = float_path(torch.float64)
    ref32 = float_path(torch.float32)
    n3, e3 = copy.deepcopy(net).to(DEV), copy.deepcopy(enc).to(DEV)
    s3 = sh.clone().to(DEV).requires_grad_(True)
    bits = _dev(M.pack_bits(dyn))
    _lib.variant_hits_reset(DEV)
    logits, last = n3.forward_bits(n3.project_static(s3), bits, e3, dec.to(DEV), hh.to(DEV))
    ((logits * g.to(DEV)).sum() + (last * ghh.to(DEV)).sum()).backward()
    assert len(_keys(0)) == 1 and len(_keys(1)) == 1                               # the kernel ran, forward and backward
    got = (logits.detach().double().cpu().numpy(), last.detach().double().cpu().numpy(), _named_grads(n3, e3, {"static_hidden": s3.grad}))
    assert sorted(got[2]) == sorted(want[2]) and len(got[2]) == 8 + 2 + 1
    for name, a, w, r in [("logits", got[0], want[0], ref32[0]), ("last_hh", got[1], want[1], ref32[1])] + \
            [(n, got[2][n], want[2][n], ref32[2][n]) for n in sorted(want[2])]:
        e, err = float(np.abs(r - w).max()), float(np.abs(a - w).max())
        print("forward_bits %s: err %.3g e_ref %.3g max|want| %.3g" % (name, err, e, np.abs(w).max()))
        assert np.abs(w).max() > 0 and err <= M.tolerance(e, w), (name, err, e)


def test_lean_episode_equals_the_teacher_forced_reference_path():
    """c2's window (n = 10, W = 5, H = 50), B = 64, He = Hd = 128: a lean stepper with a forward_bits scorer and a greedy
    head; then its tour replayed on an expanding stepper through DynamicBitsEncoder + forward in float64 (the wanted
    values) and float32 (e_ref) -- teacher-forced, so near-ties cannot split the tours"""
    n, B, H = 10, 64, 128
    static, dynamic = synth.rand_instances(B, n, 2, seed=91)
    static, dynamic = static.to(DEV).contiguous(), dynamic.to(DEV).contiguous()
    rows, nR = int(dynamic.shape[1]), int(dynamic.shape[2])
    assert (rows, nR) == (30, 20)
    torch.manual_seed(92)
    net = _xavier_(tools.Pointer(H, H, 'shape_heightmap', 'bot')).eval().to(DEV)
    enc = T.DynamicBitsEncoder(rows, H).to(DEV)
    sh = torch.randn(B, H, nR, device=DEV)
    dec = torch.randn(n, B, H, 1, device=DEV)
    hh0 = torch.zeros(1, B, H, device=DEV)

    def stepper(lean):
        env = T.BatchedContainer(B, [5, 50], n, "C+P+S-lb-soft", "diff", device=DEV)
        return T.EpisodeStepper(static, dynamic, env, 'bot', True, steps=n, expand_dynamic=not lean)
    sp = stepper(True)
    state = {"hh": hh0, "logits": [], "last": []}

    def scorer(step, **_):
        logits, state["hh"] = net.forward_bits(proj, sp.dynamic_bits, enc, dec[step], state["hh"])
        state["logits"].append(logits.clone())
        state["last"].append(state["hh"].clone())
        return logits
    with torch.no_grad():
        proj = net.project_static(sh)
        _lib.variant_hits_reset(DEV)
        out = T.run_episode(static, dynamic, T.PointerHeadPolicy(scorer, greedy=True), 5, 50, stepper=sp, check=False)
    assert sp.dynamic is None and sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == _lib.TAP_HIT_POINTER) == n
    tour = out["tour_idx"]

    class Watch(object):
        """TapePolicy that runs the reference path on the expanded `dynamic` of every step, in two precisions"""

        def __init__(self):
            self.tape = T.TapePolicy(tour)
            self.nets = {d: (copy.deepcopy(net).to(d), copy.deepcopy(enc).to(d)) for d in (torch.float64, torch.float32)}
            self.hh = {d: hh0.to(d) for d in self.nets}
            self.rec = {d: [] for d in self.nets}

        def __call__(self, step, dynamic, **kw):
            for d, (n2, e2) in self.nets.items():
                logits, self.hh[d] = n2(sh.to(d), e2(dynamic.to(d)), dec[step].to(d), self.hh[d])
                self.rec[d].append((logits.double().cpu().numpy(), self.hh[d].double().cpu().numpy()))
            return self.tape(step=step)
    watch = Watch()
    sp2 = stepper(False)
    with torch.no_grad():
        out2 = T.run_episode(static, dynamic, watch, 5, 50, stepper=sp2, check=False)
    assert torch.equal(out2["tour_idx"], tour) and torch.equal(out2["reward"], out["reward"])
    for t in range(n):
        for name, a, i in (("logits", state["logits"][t], 0), ("last_hh", state["last"][t], 1)):
            w, r = watch.rec[torch.float64][t][i], watch.rec[torch.float32][t][i]
            e, err = float(np.abs(r - w).max()), float(np.abs(a.double().cpu().numpy() - w).max())
            print("episode step %d %s: err %.3g e_ref %.3g" % (t, name, err, e))
            assert err <= M.tolerance(e, w), (t, name, err, e)


def test_forward_bits_step_replays_from_a_hip_graph():
    B, rows, nR, H = 64, 30, 20, 128
    torch.manual_seed(41)
    net = _xavier_(tools.Pointer(H, H, 'shape_heightmap', 'bot')).eval().to(DEV)
    enc = T.DynamicBitsEncoder(rows, H).to(DEV)
    bits = _dev(M.pack_bits(np.random.RandomState(42).rand(B, rows, nR) < 0.1))
    sh, dec, hh = torch.randn(B, H, nR, device=DEV), torch.randn(B, H, 1, device=DEV), torch.randn(1, B, H, device=DEV)
    with torch.no_grad():
        proj = net.project_static(sh)
        eager = net.forward_bits(proj, bits, enc, dec, hh)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            net.forward_bits(proj, bits, enc, dec, hh)
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = net.forward_bits(proj, bits, enc, dec, hh)
        for _ in range(2):
            rec[0].zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(rec[0], eager[0]) and torch.equal(rec[1], eager[1])
    assert bool(torch.isfinite(eager[0]).all()) and float(eager[0].abs().max()) > 0
