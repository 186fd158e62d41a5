"""The pointer network's static-rows form on the MI355X (pointer.hip: k_pointer_scores<HPL, SS>, k_pointer_scores_bw<HPL, SS>
with SS = 0, 2, 3, 4; tapenv.h: tap_pointer_scores_static) against the float64 model of tests/pointer_static_model.py, and
against the ``proj`` form byte for byte.

The tolerance is pointer_model.tolerance(e_ref, want) = 4 e_ref + 16 * 2^-24 * max |want|, with e_ref the largest
float32-vs-float64 error of the reference's own torch form on the CPU, the static encoder's convolution included (for the
gradients: of float32 torch autograd of the folded model).  The kernel's inputs are the float64 fold rounded to float32 and
``want`` is the float64 model ON those rounded inputs.  Each test prints its figures before it asserts.

The byte test needs no tolerance: with G and g multiples of 2^-10 in [-1, 1] and xs integers in 1 .. 8 every partial sum of
P = g + G . xs is a multiple of 2^-10 below 2^7 -- 17 bits --, so P is exact in float32 in any order; that P, laid out as
``proj``, must make the ``proj`` form write the bytes the static-rows form writes."""
import copy

import numpy as np
import pytest
import torch

import actor_reference_cases as AC
import pointer_model as M
import pointer_static_model as SM
import tap_net_amd as T
from tap_net_amd import _lib, rollout, synth, tools

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (rows, nR, Hd, S, B): test_pointer_gpu's axes -- both shadow planes, HPL 1 and 2, 1 / 2 / 4 hidden chunks, nR below and
# above 64, one and two envs per workgroup with a full (2050) and a ragged (2051) last workgroup -- and every S path the
# kernel distinguishes: G in registers for S = 2, 3, 4 (one instantiation each) and the LDS copy for the rest, at its
# smallest (1) and largest (8) S with one hidden row per lane and -- the last case, which the other axes do not need -- at
# S = 5 with two
CASES = [(10, 4, 64, 2, 1), (30, 20, 128, 2, 67), (30, 60, 128, 3, 3), (63, 68, 64, 4, 3), (65, 20, 128, 3, 3), (126, 60, 256, 3, 2),
         (128, 256, 64, 8, 3), (30, 20, 128, 2, 2050), (10, 4, 64, 1, 2051), (30, 20, 128, 5, 3)]
DENSITIES = (0.0, 0.1, 1.0)
BW_CASES = [(30, 20, 128, 2, 67), (65, 68, 64, 4, 3), (126, 60, 256, 3, 2), (10, 4, 64, 2, 2050), (10, 4, 64, 1, 2051),
            (30, 20, 128, 5, 3)]


def _geom(rows, Hd):
    planes = M.planes_of(rows)
    hpl = 2 if planes == 1 and Hd > 64 else 1
    return hpl, planes, Hd // (64 * hpl)


def _ss(S):
    """the instantiation that takes S static rows: S itself in registers for 2, 3, 4, else the LDS copy (0)"""
    return S if 2 <= S <= 4 else 0


def _epb(B):
    return max(1, B // 1024)


def _keys(extra):
    return {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_POINTER and k[5] == extra}


def _key(rows, Hd, extra, S):
    return (_lib.TAP_HIT_POINTER, 0) + _geom(rows, Hd) + (extra, S)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))


def _inputs(rows, nR, Hd, S, B, density, seed):
    """-> X, the kernel's float32 inputs (xs, G, g, M, k, q, va, vp), the shadow"""
    X = SM.make_case(B, rows, nR, Hd, Hd, S, density, seed)
    G, g, Mf, k, q = (np.asarray(a, np.float32) for a in SM.fold(X, np.float64))
    return X, (X["xs"], G, g, Mf, k, q, X["va"], X["vp"]), M.pack_bits(X["dyn"])


def _raw(inp, bits, rows):
    """the static-rows forward entry on device copies -> logits, attn, t as numpy"""
    B, _, nR = inp[0].shape
    Hd = inp[5].shape[1]
    out = [torch.full(s, float('nan'), device=DEV) for s in ((B, nR), (B, nR), (B, Hd))]
    rollout._scores_static_into(*(_dev(a) for a in inp[:1]), _dev(bits), *(_dev(a) for a in inp[1:]), rows, *out)
    return [o.cpu().numpy() for o in out]


def _raw_proj(proj, inp, bits, rows):
    """the ``proj`` form's forward entry on ``proj`` (B, 3 Hd, nR) and the static case's other inputs"""
    B, H3, nR = proj.shape
    out = [torch.full(s, float('nan'), device=DEV) for s in ((B, nR), (B, nR), (B, H3 // 3))]
    rollout._scores_into(_dev(M.to_layout(proj)), _dev(bits), *(_dev(a) for a in inp[3:]), rows, *out)
    return [o.cpu().numpy() for o in out]


def _raw_backward(inp, bits, rows, attn, t, grad, proj=None):
    """the backward entry of the static-rows form, or with ``proj`` (B, 3 Hd, nR) of the ``proj`` form -> dU, dq, dva, dvp"""
    xs, G, g, Mf, k, q, va, vp = inp
    B, S, nR = xs.shape
    Hd = q.shape[1]
    L, c = _lib.lib(), _lib.ctx(torch.device(DEV))
    out = [torch.full(s, float('nan'), device=DEV) for s in ((B, 3 * Hd, nR), (B, Hd), (Hd,), (Hd,))]
    d = {n: _dev(a) for n, a in (("bits", bits), ("M", Mf), ("k", k), ("q", q), ("va", va), ("vp", vp), ("attn", attn), ("t", t),
                                 ("grad", grad))}
    tail = [_lib.ptr(d[n]) for n in ("M", "k", "q", "va", "vp", "attn", "t", "grad")] + [_lib.ptr(o) for o in out]
    st = _lib.stream_of(torch.device(DEV))
    if proj is None:
        need = int(L.tap_pointer_scores_static_backward_scratch(B, nR, rows, Hd, S))
        scratch = torch.empty(max(need, 16) // 4, device=DEV)
        dx, dG, dg = _dev(xs), _dev(G), _dev(g)
        _lib.check(L.tap_pointer_scores_static_backward(c, _lib.ptr(dx), _lib.ptr(d["bits"]), B, nR, rows, Hd, S, _lib.ptr(dG),
                                                        _lib.ptr(dg), *tail, _lib.ptr(scratch), need, st), c)
    else:
        need = int(L.tap_pointer_scores_backward_scratch(B, nR, rows, Hd))
        scratch = torch.empty(max(need, 16) // 4, device=DEV)
        dp = _dev(M.to_layout(proj))
        _lib.check(L.tap_pointer_scores_backward(c, _lib.ptr(dp), _lib.ptr(d["bits"]), B, nR, rows, Hd, *tail, _lib.ptr(scratch),
                                                 need, st), c)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _e_ref(X):
    with torch.no_grad():
        r32, r64 = SM.reference_form_torch(X, torch.float32), SM.reference_form_torch(X, torch.float64)
    return [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)]


def test_case_list_covers_every_axis():
    """from the launch record of one call per case (zero inputs: only the geometry matters)"""
    seen = set()
    for rows, nR, Hd, S, B in CASES:
        _lib.variant_hits_reset(DEV)
        z = lambda *s: torch.zeros(*s, device=DEV)
        bits = torch.zeros(B, M.planes_of(rows) * nR, dtype=torch.int64, device=DEV)
        with torch.no_grad():
            out = T.pointer_scores_static(z(B, S, nR), bits, z(3 * Hd, S), z(3 * Hd), z(3 * Hd, rows), z(3 * Hd), z(B, Hd), z(Hd), z(Hd))
        assert tuple(out.shape) == (B, nR) and not bool(out.any())
        keys = _keys(0)
        assert keys == {_key(rows, Hd, 0, S)}, keys
        seen |= keys
    assert {k[3] for k in seen} == {1, 2}                                          # both shadow planes
    assert {(k[2], k[3]) for k in seen} == {(1, 1), (2, 1), (1, 2)}                # every (HPL, PLANES) the launcher can pick
    assert {k[4] for k in seen} == {1, 2, 4}                                       # one and several hidden chunks
    assert {_ss(k[6]) for k in seen} == {0, 2, 3, 4}                               # every S path: registers for 2, 3, 4, else LDS
    assert {k[6] for k in seen if _ss(k[6]) == 0} == {1, 5, 8}                     # the LDS copy at its smallest and largest S
    assert {(k[2], _ss(k[6]) > 0) for k in seen} == {(1, True), (2, True), (1, False), (2, False)}   # both with either HPL
    assert {(k[2], _ss(k[6]) > 0) for k in seen if (k[2], k[3], k[4]) in {_geom(c[0], c[2]) for c in BW_CASES}} == \
        {(1, True), (2, True), (1, False), (2, False)}
    assert {c[2] for c in CASES} == {64, 128, 256}
    assert min(c[1] for c in CASES) < 64 < max(c[1] for c in CASES) and {c[1] for c in CASES} >= {4, 20, 60, 68, 256}
    assert any(_epb(c[4]) > 1 and c[4] % _epb(c[4]) for c in CASES)                # a ragged last workgroup
    assert any(_epb(c[4]) > 1 and c[4] % _epb(c[4]) == 0 for c in CASES) and any(_epb(c[4]) == 1 and c[4] > 1 for c in CASES)
    assert {_ss(c[3]) for c in BW_CASES} == {0, 2, 3, 4}                           # the backward's cases take every S path too


@pytest.mark.parametrize("rows,nR,Hd,S,B", CASES)
def test_forward(rows, nR, Hd, S, B):
    worst = 0.0
    for i, density in enumerate(DENSITIES):
        X, inp, bits = _inputs(rows, nR, Hd, S, B, density, 1000 * rows + 10 * nR + i)
        with torch.no_grad():
            want = [w.numpy() for w in SM.folded_torch(_t64(inp[0]), _t64(inp[1]), _t64(inp[2]), _t64(X["dyn"]), *(_t64(a) for a in inp[3:]))]
        e_ref = _e_ref(X)
        _lib.variant_hits_reset(DEV)
        got = _raw(inp, bits, rows)
        assert _keys(0) == {_key(rows, Hd, 0, S)}
        for name, g, w, e in zip(("logits", "attn", "t"), got, want, e_ref):
            assert g.dtype == np.float32 and g.shape == w.shape and np.isfinite(g).all()
            err = float(np.abs(g.astype(np.float64) - w).max())
            print("pointer static forward %s density %.1f %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
                  % ((rows, nR, Hd, S, B), density, name, err, e, _ratio(err, e), np.abs(w).max()))
            assert err <= M.tolerance(e, w), (name, density, err, e)
            worst = max(worst, _ratio(err, e))
        assert abs(got[1].sum(1) - 1).max() <= 1e-5                                # attn is a softmax over ALL columns
        again = _raw(inp, bits, rows)
        junk = _raw(inp, M.garbage(bits, rows, nR, 7), rows)
        for a, b, c in zip(got, again, junk):
            assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes()
    print("pointer static forward %s: worst err / e_ref %.2f" % ((rows, nR, Hd, S, B), worst))


def _grads_torch(inp, dyn, grad, dtype):
    """autograd of the folded model in torch on the CPU -> dP (= dU), dG, dg, dM, dk, dq, dva, dvp"""
    xs = torch.from_numpy(np.asarray(inp[0])).to(dtype)
    leaves = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in inp[1:]]
    P = leaves[1][None, :, None] + torch.einsum('xs,bsc->bxc', leaves[0], xs)
    P.retain_grad()
    logits = M.folded_torch(P, torch.from_numpy(dyn).to(dtype), *leaves[2:])[0]
    (logits * torch.from_numpy(grad).to(dtype)).sum().backward()
    return [P.grad.double().numpy()] + [v.grad.double().numpy() for v in leaves]


def _grads_device(inp, bits, grad, rows):
    """through the autograd function -> dG, dg, dM, dk, dq, dva, dvp"""
    xs = _dev(inp[0])
    leaves = [_dev(a).requires_grad_(True) for a in inp[1:]]
    mine = _dev(bits)
    logits = T.pointer_scores_static(xs, mine, *leaves, rows=rows)
    assert logits.requires_grad
    mine.fill_(-1)                                                                 # the caller's shadow is overwritten before the backward
    logits.backward(_dev(grad))
    assert xs.grad is None
    return [v.grad.cpu().numpy() for v in leaves]


def _exact_inputs(rows, nR, Hd, S, B, seed):
    """the byte test's inputs: G, g multiples of 2^-10 in [-1, 1] and xs integers in 1 .. 8; everything else arbitrary"""
    X, inp, bits = _inputs(rows, nR, Hd, S, B, 0.1, seed)
    rng = np.random.RandomState(seed + 1)
    G = (rng.randint(-1024, 1025, size=(3 * Hd, S)) / 1024.0).astype(np.float32)
    g = (rng.randint(-1024, 1025, size=(3 * Hd,)) / 1024.0).astype(np.float32)
    xs = rng.randint(1, 9, size=(B, S, nR)).astype(np.float32)
    P = SM.static_term(xs, G, g, np.float32)
    # the premise: float32 arithmetic was exact, so a fused and an unfused chain in any order give this P
    assert P.dtype == np.float32 and np.array_equal(P.astype(np.float64), SM.static_term(xs, G, g, np.float64))
    return X, (xs, G, g) + inp[3:], bits, P


@pytest.mark.parametrize("rows,nR,Hd,S,B", CASES)
def test_same_bytes_as_the_proj_form(rows, nR, Hd, S, B):
    X, inp, bits, P = _exact_inputs(rows, nR, Hd, S, B, 500 * rows + nR + S)
    got, want = _raw(inp, bits, rows), _raw_proj(P, inp, bits, rows)
    for name, a, b in zip(("logits", "attn", "t"), got, want):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes(), name
    assert np.abs(got[0]).max() > 0
    grad = np.random.RandomState(rows + B).randn(B, nR).astype(np.float32)
    _lib.variant_hits_reset(DEV)
    mine = _raw_backward(inp, bits, rows, got[1], got[2], grad)
    theirs = _raw_backward(inp, bits, rows, got[1], got[2], grad, proj=P)
    assert _keys(1) == {_key(rows, Hd, 1, S), _key(rows, Hd, 1, 0)}
    for name, a, b in zip(("dU", "dq"), mine, theirs):
        assert np.isfinite(a).all() and np.abs(a).max() > 0 and a.tobytes() == b.tobytes(), name
    if mine[2].tobytes() != theirs[2].tobytes() or mine[3].tobytes() != theirs[3].tobytes():
        # sums of one partial per workgroup: another count of envs per workgroup rounds them differently; both forms
        # are then held to the backward test's rule
        want64, ref32 = _grads_torch(inp, X["dyn"], grad, torch.float64), _grads_torch(inp, X["dyn"], grad, torch.float32)
        for name, i, j in (("dva", 2, 6), ("dvp", 3, 7)):
            e = float(np.abs(ref32[j] - want64[j]).max())
            for form, out in (("static", mine), ("proj", theirs)):
                err = float(np.abs(out[i].astype(np.float64) - want64[j]).max())
                print("byte test %s %s %s: err %.3g e_ref %.3g" % ((rows, nR, Hd, S, B), form, name, err, e))
                assert err <= M.tolerance(e, want64[j]), (form, name, err, e)


@pytest.mark.parametrize("rows,nR,Hd,S,B", BW_CASES)
def test_backward(rows, nR, Hd, S, B):
    X, inp, bits = _inputs(rows, nR, Hd, S, B, 0.1, 77 * rows + nR + S)
    grad = np.random.RandomState(rows + B).randn(B, nR).astype(np.float32)
    want = _grads_torch(inp, X["dyn"], grad, torch.float64)
    ref32 = _grads_torch(inp, X["dyn"], grad, torch.float32)
    fwd = _raw(inp, bits, rows)
    _lib.variant_hits_reset(DEV)
    raw = _raw_backward(inp, bits, rows, fwd[1], fwd[2], grad)
    got = _grads_device(inp, bits, grad, rows)
    assert _keys(1) == {_key(rows, Hd, 1, S)} and _keys(0) == {_key(rows, Hd, 0, S)}
    rows_ = [("raw dU", raw[0], want[0], ref32[0]), ("raw dq", raw[1], want[5], ref32[5]), ("raw dva", raw[2], want[6], ref32[6]),
             ("raw dvp", raw[3], want[7], ref32[7])] + \
        [(n, a, w, r) for n, a, w, r in zip(("dG", "dg", "dM", "dk", "dq", "dva", "dvp"), got, want[1:], ref32[1:])]
    worst = 0.0
    for name, a, w, r in rows_:
        assert a.dtype == np.float32 and a.shape == w.shape and np.isfinite(a).all(), name
        e = float(np.abs(r - w).max())
        err = float(np.abs(a.astype(np.float64) - w).max())
        print("pointer static backward %s %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
              % ((rows, nR, Hd, S, B), name, err, e, _ratio(err, e), np.abs(w).max()))
        assert np.abs(w).max() > 0 and err <= M.tolerance(e, w), (name, err, e)
        worst = max(worst, _ratio(err, e))
    print("pointer static backward %s: worst err / e_ref %.2f" % ((rows, nR, Hd, S, B), worst))
    for a, b in zip(raw, _raw_backward(inp, bits, rows, fwd[1], fwd[2], grad)):     # deterministic: the same bytes
        assert a.tobytes() == b.tobytes()
    for a, b in zip(got, _grads_device(inp, bits, grad, rows)):
        assert a.tobytes() == b.tobytes()


# ---- through the modules -----------------------------------------------------------------------------------------------
def _actor(He, Hd, S, rows, seed):
    torch.manual_seed(seed)
    net = tools.Pointer(He, Hd, 'shape_heightmap', 'bot').eval()
    for p in net.parameters():
        torch.nn.init.xavier_uniform_(p) if p.dim() > 1 else torch.nn.init.normal_(p, std=0.1)
    return dict(pointer=net, dynamic_encoder=T.DynamicBitsEncoder(rows, He).eval(), static_encoder=torch.nn.Conv1d(S, He, 1),
                static_decoder=torch.nn.Conv1d(2, Hd // 2, 1), dynamic_decoder=torch.nn.Conv1d(4, Hd // 2, 1))


def _named_grads(mods):
    return {"%s.%s" % (m, n): p.grad.detach().double().cpu().numpy() for m, mod in mods.items() for n, p in mod.named_parameters()}


def _saved_tensors(root):
    """every tensor that the autograd graph below ``root`` keeps for the backward"""
    seen, stack, out = set(), [root.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        out += [t for t in getattr(fn, "saved_tensors", ()) if torch.is_tensor(t)]
        out += [getattr(fn, a) for a in dir(fn) if a.startswith("_saved_") and torch.is_tensor(getattr(fn, a))]
        stack += [nxt for nxt, _ in fn.next_functions]
    return out


def test_three_training_steps_through_the_modules():
    """c2's window, B = 67, an EpisodeStepper(expand_dynamic=False): fold_static once, three steps of forward_step with the
    head and ONE backward(), against the float64 CPU modules -- off the GPU the record is ``forward`` on
    ``static_encoder(xs)`` -- teacher-forced on the device's picks, with their float32 run as e_ref"""
    B, n, He, Hd, steps = 67, 10, 128, 128, 3
    static, dynamic = synth.rand_instances(B, n, 2, seed=71)
    static, dynamic = static.to(DEV).contiguous(), dynamic.to(DEV).contiguous()
    rows, nR = int(dynamic.shape[1]), int(dynamic.shape[2])
    assert (rows, nR) == (30, 20)
    mods = _actor(He, Hd, 2, rows, 72)
    rng = np.random.RandomState(73)
    u, adv = rng.rand(steps, B).astype(np.float32), rng.randn(B).astype(np.float32)
    dev = {k: copy.deepcopy(m).to(DEV) for k, m in mods.items()}
    net = dev["pointer"]
    env = T.BatchedContainer(B, [5, 50], n, "C+P+S-lb-soft", "diff", device=DEV)
    seen, logps, hh = [], [], None
    _lib.variant_hits_reset(DEV)
    with torch.enable_grad():
        sp = T.EpisodeStepper(static, dynamic, env, steps=steps, expand_dynamic=False)
        sp.begin(static, dynamic)
        sf = net.fold_static(dev["static_encoder"], static[:, 1:, :])
        fold = net.fold_episode(dev["dynamic_encoder"], *net.fold_decoder(dev["static_decoder"], dev["dynamic_decoder"]))
        for k in range(steps):
            rec = [t.detach().clone().cpu() for t in (sp.dynamic_bits, sp.current_mask, sp.decoder_static, sp.decoder_dynamic)]
            logits, hh = net.forward_step(sf, sp.dynamic_bits, fold, sp.decoder_static, sp.decoder_dynamic, hh)
            ptr, logp = T.pointer_pick(logits, sp.current_mask, _dev(u[k]))
            seen.append(rec + [ptr.cpu(), logits.detach().double().cpu().numpy()])
            logps.append(logp)
            sp.step(ptr)
        loss = (_dev(adv) * torch.stack(logps, 1).sum(1)).sum()
        kept = _saved_tensors(loss)
        loss.backward()
    sp.check()
    hits = _lib.variant_hits(DEV)
    count = lambda pred: sum(v for key, v in hits.items() if pred(key))
    assert count(lambda key: key[0] == _lib.TAP_HIT_DECODER and key[5] == 0) == steps      # one decoder launch per step
    assert count(lambda key: key[0] == _lib.TAP_HIT_POINTER and key[5] == 0 and key[6] == 2) == steps   # one static-rows launch
    assert count(lambda key: key[0] == _lib.TAP_HIT_POINTER and key[6] == 0) == 0           # and no proj-form launch at all
    assert count(lambda key: key[0] == _lib.TAP_HIT_POINTER and key[5] == 1 and key[6] == 2) == steps
    # nothing of size Hd x columns per env is kept for the backward: no proj, no static_hidden, no dU
    assert kept and max(t.numel() for t in kept) < B * nR * Hd, max(t.numel() for t in kept)
    got = _named_grads(dev)

    def cpu_run(dtype):
        ms = {k: copy.deepcopy(m).to(dtype) for k, m in mods.items()}
        net = ms["pointer"]
        sf = net.fold_static(ms["static_encoder"], static[:, 1:, :].cpu().to(dtype))
        fold = net.fold_episode(ms["dynamic_encoder"], *net.fold_decoder(ms["static_decoder"], ms["dynamic_decoder"]))
        hh, logps, out = None, [], []
        for k in range(steps):
            bits, cur, ds, dd, ptr, _ = seen[k]
            dyn = torch.from_numpy(M.unpack_bits(bits.numpy(), rows, nR)).to(dtype)
            logits, hh = net.forward_step(sf, dyn, fold, ds.to(dtype), dd.to(dtype), hh)
            logps.append(torch.log_softmax(logits + torch.log(cur.to(dtype)), dim=1).gather(1, ptr.unsqueeze(1))[:, 0])
            out.append(logits.detach().double().numpy())
        (torch.from_numpy(adv).to(dtype) * torch.stack(logps, 1).sum(1)).sum().backward()
        return out, _named_grads(ms)
    want, ref32 = cpu_run(torch.float64), cpu_run(torch.float32)
    assert sorted(got) == sorted(want[1]) and len(got) == 8 + 2 + 2 + 2 + 2
    rows_ = [("logits %d" % k, seen[k][5], want[0][k], ref32[0][k]) for k in range(steps)] + \
        [(name, got[name], want[1][name], ref32[1][name]) for name in sorted(got)]
    failed = []
    for name, a, w, r in rows_:
        e, err = float(np.abs(r - w).max()), float(np.abs(a - w).max())
        print("static modules %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g" % (name, err, e, _ratio(err, e), np.abs(w).max()))
        if not (np.abs(w).max() > 0 and err <= M.tolerance(e, w)):
            failed.append((name, err, e))
    assert not failed, failed


@pytest.mark.parametrize("D,ws", AC.CASES)
def test_the_references_actor(D, ws):
    """INTEGRATION 2i / 2j's recipe with fold_static in place of project_static, teacher-forced on the recorded tour, ONE
    backward() of L = sum_b adv[b] sum_t tour_logp[b, t]: per-step logits and last_hh, tour_logp and every parameter's
    gradient within 4 e_ref + 16 ulp of the recorded float64 numbers, with the fixture's own e_ref"""
    import test_actor_reference_gpu as ARG
    z = AC.load(D, ws)
    B, n = AC.BATCH[D], AC.N
    st, dy = AC.instances(D)
    static, dynamic = _dev(st), _dev(dy)
    mods, _ = AC.build(z, D)
    for m in mods.values():
        m.to(DEV)
    enc, dec_s, dec_d, pointer = mods["dynamic_encoder."], mods["static_decoder.conv."], AC.dynamic_decoder(mods), mods["pointer."]
    env = T.BatchedContainer(B, AC.CONTAINER[D], n, "C+P+S-lb-soft", "diff", device=DEV)
    state = {"hh": None, "last_hh": []}

    def scorer(step, decoder_static, decoder_dynamic):
        logits, state["hh"] = pointer.forward_step(state["sf"], sp.dynamic_bits, state["fold"], decoder_static, decoder_dynamic, state["hh"])
        state["last_hh"].append(state["hh"])
        return logits
    _lib.variant_hits_reset(DEV)
    with torch.enable_grad():
        sp = T.EpisodeStepper(static, dynamic, env, steps=n, expand_dynamic=False)
        state["sf"] = pointer.fold_static(mods["static_encoder.conv."], static[:, 1:, :])
        state["fold"] = pointer.fold_episode(enc, *pointer.fold_decoder(dec_s, dec_d, combine='cat'))
        pol = ARG._RecordedTour(scorer, _dev(z["tour_idx"].astype(np.int64).T))
        T.run_episode(static, dynamic, pol, 5, 50, stepper=sp, check=False)
        tour_logp = torch.stack(pol.logp, dim=1)
        (_dev(z["adv"]).double() * tour_logp.sum(1)).sum().backward()
    sp.check()
    hits = _lib.variant_hits(DEV)
    pointer_hits = {key[5:]: v for key, v in hits.items() if key[0] == _lib.TAP_HIT_POINTER}
    assert pointer_hits == {(0, D): n, (1, D): n}, pointer_hits                     # S = D static rows; no proj-form launch
    cpu = lambda t: t.detach().double().cpu().numpy()
    label = "static actor %dD %s" % (D, ws)
    ARG._held(label, [("logits %d" % k, cpu(pol.logits[k]), z["logits"][k], z["e_ref_logits"][k]) for k in range(n)] +
              [("last_hh %d" % k, cpu(state["last_hh"][k])[0], z["last_hh"][k], z["e_ref_last_hh"][k]) for k in range(n)] +
              [("tour_logp", cpu(tour_logp), z["tour_logp"], z["e_ref_tour_logp"])])
    params = AC.named_parameters(mods)
    assert len(params) == AC.N_KEYS[D] and all(p.grad is not None for p in params.values())
    ARG._held(label + " gradient", [(k, cpu(p.grad), z["grad_" + k], z["e_ref_grad_" + k]) for k, p in sorted(params.items())])


def test_fold_and_two_steps_replay_from_a_hip_graph():
    B, rows, nR, H, S = 64, 30, 20, 128, 2
    mods = {k: m.to(DEV) for k, m in _actor(H, H, S, rows, 61).items()}
    net = mods["pointer"]
    rng = np.random.RandomState(62)
    bits = [_dev(M.pack_bits(rng.rand(B, rows, nR) < 0.1)) for _ in range(2)]
    mask = _dev((rng.rand(B, nR) < 0.5).astype(np.float32))
    mask[:, 0] = 1
    u = _dev(rng.rand(B).astype(np.float32))
    static = _dev(np.concatenate((np.zeros((B, 1, nR)), rng.randint(1, 9, size=(B, S, nR))), 1).astype(np.float32))
    hh = torch.tanh(torch.randn(1, B, H, device=DEV))
    ds, dd = torch.randint(0, 6, (B, 2, 1), device=DEV).float(), torch.randint(0, 51, (B, 4, 1), device=DEV).float()

    def episode():
        sf = net.fold_static(mods["static_encoder"], static[:, 1:, :])
        fold = net.fold_episode(mods["dynamic_encoder"], *net.fold_decoder(mods["static_decoder"], mods["dynamic_decoder"]))
        out, last = [], hh
        for k in range(2):
            logits, last = net.forward_step(sf, bits[k], fold, ds, dd, last)
            ptr, logp = T.pointer_pick(logits, mask, u)
            out += [logits, last, ptr, logp]
        return out
    with torch.no_grad():
        _lib.variant_hits_reset(DEV)
        eager = episode()
        assert sum(v for key, v in _lib.variant_hits(DEV).items() if key[0] == _lib.TAP_HIT_POINTER and key[6] == S) == 2
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            episode()
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = episode()
        for _ in range(2):
            for v in rec:
                v.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(rec, eager):
                assert torch.equal(a, b)
    assert bool(torch.isfinite(eager[0]).all()) and float(eager[0].abs().max()) > 0 and not torch.equal(eager[0], eager[4])


def test_statuses_in_the_headers_order():
    """the C entries on the device's own context and buffers: bad dimensions, an empty batch, a null buffer, an unsupported
    shape (S = 9, Hd = 96), a short scratch, a misaligned dU -- each refused before anything is launched"""
    L, c = _lib.lib(), _lib.ctx(torch.device(DEV))
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED
    buf = torch.zeros(1 << 16, device=DEV)
    p, st = buf.data_ptr(), _lib.stream_of(torch.device(DEV))
    _lib.variant_hits_reset(DEV)

    def fwd(B, nR, rows, Hd, S, bufs=None):
        b = [p] * 12 if bufs is None else bufs
        return L.tap_pointer_scores_static(c, b[0], b[1], B, nR, rows, Hd, S, *b[2:12], st)

    def bwd(B, nR, rows, Hd, S, bufs=None, scr=p, nbytes=1 << 18):
        b = [p] * 16 if bufs is None else bufs
        return L.tap_pointer_scores_static_backward(c, b[0], b[1], B, nR, rows, Hd, S, *b[2:16], scr, nbytes, st)
    for f, nbuf in ((fwd, 12), (bwd, 16)):
        assert f(-1, 20, 30, 128, 2) == inv and f(2, 0, 30, 128, 2) == inv and f(2, 20, 30, 128, 0) == inv       # dimensions first
        assert f(0, 20, 30, 96, 9, [None] * nbuf) == ok                                                       # then the empty batch
        for hole in range(nbuf):
            args = [p] * nbuf
            args[hole] = None
            assert f(2, 20, 30, 96, 9, args) == inv                                                          # a null buffer before the shape
        assert f(2, 20, 30, 128, 9) == uns and f(2, 20, 30, 96, 2) == uns and f(2, 22, 30, 128, 2) == uns
    need = int(L.tap_pointer_scores_static_backward_scratch(2, 20, 30, 128, 2))
    assert need > 0 and bwd(2, 20, 30, 128, 2, nbytes=need - 1) == inv and bwd(2, 20, 30, 128, 2, scr=None, nbytes=need) == inv
    assert bwd(2, 20, 30, 96, 9, nbytes=0) == uns                                                              # the shape before the scratch
    args = [p] * 16
    args[12] = p + 8                                                                                           # dU leaves as float4s
    assert bwd(2, 20, 30, 128, 2, args) == inv
    args = [p] * 12
    args[1] = p + 4                                                                                            # the shadow's words are 8 bytes
    assert fwd(2, 20, 30, 128, 2, args) == inv
    torch.cuda.synchronize()
    assert not [k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_POINTER]                             # nothing was launched
