"""The launch geometries that pointer.hip, encode.hip and critic.hip take at large batches, on the MI355X: 3, 4, 5 and 8
consecutive envs per workgroup (8 is the benchmark's B = 8192), every result of the loop that halves that count while the
LDS exceeds its budget, ragged last workgroups at each, and the second level of the ordered reduces (more than 32 partials).
tests/launch_geometry_cases.py has the shapes; the class of each is read from the library (tap_pointer_scores_geometry,
tap_encode_bits_geometry), and tests/test_launch_geometry_cpu.py checks without a GPU that the list reaches every class.

What a pointer case asserts, for the ``proj`` form and the static-rows form alike:
  * every env has inputs of its own (random per env, drawn on the device), so an env that read a neighbour's LDS slot, or
    a workgroup that took the wrong run of envs, computes something else;
  * the outputs carry a workgroup's worth of canary rows behind row B, which come back untouched, and no canary is left in
    the rows below B;
  * every per-env output -- logits, attn, t; dU (which is dproj), dq -- is, byte for byte, what the same envs give when they
    are run in chunks of at most 1023, i.e. with ONE env per workgroup, the geometry that tests/test_pointer_gpu.py and
    tests/test_pointer_static_gpu.py hold to the float64 model at every shape.  No order of summation inside an env depends
    on the envs per workgroup E: the columns of an env go to the four wavefronts by column index alone, a wavefront adds its
    columns in ascending order, the wavefronts' partials are added in wavefront order (ptr_add_waves), the hidden chunks in
    chunk order, and E only moves where in the LDS an env's vectors lie;
  * on a sample of at most 64 envs -- the whole first workgroup, the whole ragged last one, and every slot of a middle one --
    the same outputs are within pointer_model.tolerance(e_ref, want) = 4 e_ref + 16 * 2^-24 * max |want| of the float64
    model, e_ref being the error of the reference's own form (the gradients: of autograd of the folded model) in float32
    torch on the CPU for those envs.  The sample's inputs are the float64 fold of a reference-form case rounded to float32,
    as in tests/test_pointer_gpu.py; the other envs' are drawn directly;
  * the sums over the batch -- dva, dvp, dM, dk, and dG, dg of the static-rows form -- do round differently with the
    geometry (one partial per workgroup, the partials in runs of 32), so on the nR = 4 cases they are held to float64
    autograd of the folded model over the WHOLE batch by the same rule, with max |want| > 0;
  * a second call gives the same bytes.
The encoder's forward is the bit-exact model of tests/dyn_encoder_model.py on all envs, its backward the bound of
tests/test_dyn_encoder_gpu.py; the critic runs the tests of tests/test_critic_gpu.py themselves at the large batches.
Each test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import dyn_encoder_model as EM
import launch_geometry_cases as LG
import pointer_model as M
import pointer_static_model as SM
import tap_net_amd as T
from tap_net_amd import _lib, rollout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 1023                    # the largest batch that runs with one env per workgroup (asserted through the query)
CANARY = 0x7FC0BEEF             # a quiet NaN with a payload: nothing the kernels compute


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _canary(*shape):
    t = torch.empty(*shape, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(CANARY)
    return t


def _i32(t):
    return t.contiguous().view(torch.int32)


def _untouched(t):
    return bool((_i32(t) == CANARY).all())


def _written(t):
    return not bool((_i32(t) == CANARY).any())


def _differing_envs(a, b):
    """the first envs whose bytes differ (empty: the same bytes)"""
    bad = (_i32(a) != _i32(b)).flatten(1).any(1).nonzero().flatten()
    return bad[:8].tolist()


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))


def _pack(dyn):
    """pointer_model.pack_bits on the device: (B, rows, nR) bool -> the shadow (B, planes * nR) int64"""
    B, rows, nR = dyn.shape
    P = M.planes_of(rows)
    out = torch.zeros(B, P, nR, dtype=torch.int64, device=dyn.device)
    for p in range(P):
        r = dyn[:, 64 * p:64 * p + 64, :].to(torch.int64)
        out[:, p, :] = (r << torch.arange(r.shape[1], device=dyn.device).view(1, -1, 1)).sum(1)
    return out.view(B, P * nR)


def _sample(B, E):
    """the whole first workgroup, every slot of a middle one, the whole ragged last one"""
    blocks = -(-B // E)
    mid = blocks // 2
    idx = sorted(set(range(min(E, B))) | set(range(mid * E, mid * E + E)) | set(range((blocks - 1) * E, B)))
    assert len(idx) <= 64 and 0 < mid < blocks - 1
    return np.array(idx)


class _Case(object):
    """a batch of B envs, each with inputs of its own; the envs of ``idx`` carry the fold of the reference-form case X"""

    def __init__(self, B, nR, rows, Hd, S, E, seed):
        self.B, self.nR, self.rows, self.Hd, self.S = B, nR, rows, Hd, S
        self.idx = idx = _sample(B, E)
        ns = len(idx)
        if S:
            self.X = X = SM.make_case(ns, rows, nR, Hd, Hd, S, 0.1, seed)
            G, g, Mf, k, q = (np.asarray(a, np.float32) for a in SM.fold(X, np.float64))
            self.small = (X["xs"], G, g, Mf, k, q, X["va"], X["vp"])
        else:
            self.X = X = M.make_case(ns, rows, nR, Hd, Hd, 0.1, seed)
            proj, Mf, k, q = (np.asarray(a, np.float32) for a in M.fold(X, np.float64))
            self.small = (proj, Mf, k, q, X["va"], X["vp"])
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        at = torch.from_numpy(idx).to(DEV)
        dyn = torch.rand(B, rows, nR, device=DEV, generator=gen) < 0.1
        dyn[at] = _dev(X["dyn"])
        self.bits = _pack(dyn)
        assert np.array_equal(self.bits[at].cpu().numpy(), M.pack_bits(X["dyn"]))
        self.dyn = dyn
        self.q = 0.5 * torch.randn(B, Hd, device=DEV, generator=gen)
        self.q[at] = _dev(q)
        if S:
            self.xs = torch.randint(1, 9, (B, S, nR), device=DEV, generator=gen).float()
            self.xs[at] = _dev(X["xs"])
            self.G, self.g = _dev(G), _dev(g)
        else:
            self.proj = 0.8 * torch.randn(B, 3, nR, Hd, device=DEV, generator=gen)
            self.proj[at] = _dev(M.to_layout(proj))
        self.M, self.k, self.va, self.vp = _dev(Mf), _dev(k), _dev(X["va"]), _dev(X["vp"])
        self.grad = torch.randn(B, nR, device=DEV, generator=gen)

    def geometry(self, B, backward):
        return _lib.pointer_scores_geometry(B, self.nR, self.rows, self.Hd, self.S, backward)

    def forward(self, lo, hi, out):
        """the forward entry on envs [lo, hi) -> out = (logits, attn, t) rows [0, hi - lo)"""
        L, c, st, p = _lib.lib(), _lib.ctx(torch.device(DEV)), _lib.stream_of(torch.device(DEV)), _lib.ptr
        n = hi - lo
        tail = [p(v) for v in (self.M, self.k, self.q[lo:hi], self.va, self.vp) + tuple(out)]
        if self.S:
            _lib.check(L.tap_pointer_scores_static(c, p(self.xs[lo:hi]), p(self.bits[lo:hi]), n, self.nR, self.rows, self.Hd, self.S,
                                                   p(self.G), p(self.g), *tail, st), c)
        else:
            _lib.check(L.tap_pointer_scores(c, p(self.proj[lo:hi]), p(self.bits[lo:hi]), n, self.nR, self.rows, self.Hd, *tail, st), c)

    def backward(self, lo, hi, attn, t, out, scratch):
        """the backward entry on envs [lo, hi) -> out = (dU, dq, dva, dvp)"""
        L, c, st, p = _lib.lib(), _lib.ctx(torch.device(DEV)), _lib.stream_of(torch.device(DEV)), _lib.ptr
        n = hi - lo
        tail = [p(v) for v in (self.M, self.k, self.q[lo:hi], self.va, self.vp, attn[lo:hi], t[lo:hi], self.grad[lo:hi]) + tuple(out)]
        if self.S:
            need = int(L.tap_pointer_scores_static_backward_scratch(n, self.nR, self.rows, self.Hd, self.S))
            _lib.check(L.tap_pointer_scores_static_backward(c, p(self.xs[lo:hi]), p(self.bits[lo:hi]), n, self.nR, self.rows, self.Hd,
                                                            self.S, p(self.G), p(self.g), *tail, p(scratch), need, st), c)
        else:
            need = int(L.tap_pointer_scores_backward_scratch(n, self.nR, self.rows, self.Hd))
            _lib.check(L.tap_pointer_scores_backward(c, p(self.proj[lo:hi]), p(self.bits[lo:hi]), n, self.nR, self.rows, self.Hd, *tail,
                                                     p(scratch), need, st), c)
        assert need == self.geometry(n, True)[1] * 2 * self.Hd * 4 and scratch.numel() * 4 >= need
        return need

    def chunks(self):
        for lo in range(0, self.B, CHUNK):
            yield lo, min(self.B, lo + CHUNK)

    def launched(self, backward):
        return {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_POINTER and k[5] == backward and k[6] == self.S}

    # ---- the float64 model and the float32 reference on the sample --------------------------------------------------
    def model_forward(self):
        """-> want (logits, attn, t) in float64 on the sample's rounded inputs, e_ref of each"""
        X, s = self.X, self.small
        with torch.no_grad():
            if self.S:
                want = SM.folded_torch(_t(s[0]), _t(s[1]), _t(s[2]), _t(X["dyn"]), *(_t(a) for a in s[3:]))
                r32, r64 = SM.reference_form_torch(X, torch.float32), SM.reference_form_torch(X, torch.float64)
            else:
                want = M.folded_torch(_t(s[0]), _t(X["dyn"]), *(_t(a) for a in s[1:]))
                r32, r64 = M.reference_form_torch(X, torch.float32), M.reference_form_torch(X, torch.float64)
        return [w.numpy() for w in want], [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)]


def _autograd(S, inp, dyn, grad, dtype):
    """autograd of the folded model on the CPU -> {name: gradient in float64}; ``inp`` as _Case.small orders it (proj in the
    contract's natural order), dU = the gradient at the static term"""
    if S:
        xs = _t(inp[0], dtype)
        G, g, Mf, k, q, va, vp = leaves = [_t(a, dtype).requires_grad_(True) for a in inp[1:]]
        P = g[None, :, None] + torch.einsum('xs,bsc->bxc', G, xs)
        P.retain_grad()
        names = ("dG", "dg", "dM", "dk", "dq", "dva", "dvp")
    else:
        P, Mf, k, q, va, vp = leaves = [_t(a, dtype).requires_grad_(True) for a in inp]
        names = ("dU", "dM", "dk", "dq", "dva", "dvp")
    logits = M.folded_torch(P, _t(dyn, dtype), Mf, k, q, va, vp)[0]
    (logits * _t(grad, dtype)).sum().backward()
    out = {n: v.grad.double().numpy() for n, v in zip(names, leaves)}
    out["dU"] = P.grad.double().numpy()
    return out


def _held(label, rows_):
    """every (name, got, want, float32 reference) within the tolerance rule; prints each figure first -> worst err / e_ref"""
    worst, failed = 0.0, []
    for name, a, w, r in rows_:
        assert a.dtype == np.float32 and a.shape == w.shape and np.isfinite(a).all(), name
        e = r if np.isscalar(r) else float(np.abs(r - w).max())
        err = float(np.abs(a.astype(np.float64) - w).max())
        print("%s %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g" % (label, name, err, e, _ratio(err, e), np.abs(w).max()))
        if not (np.abs(w).max() > 0 and err <= M.tolerance(e, w)):
            failed.append((name, err, e))
        worst = max(worst, _ratio(err, e))
    assert not failed, failed
    return worst


def _class_of(case, backward):
    """the case's class, from the library: (envs per workgroup, workgroups); the list's claim is checked against it"""
    B, nR, rows, Hd, S, (before, after) = case
    E, blocks, lds, _ = _lib.pointer_scores_geometry(B, nR, rows, Hd, S, backward)
    assert _lib.pointer_scores_geometry(B, 4, 1, 64, 0, False)[0] == before and E == after, (case, E)
    assert blocks == -(-B // E) and (E == 1 or B % E) and lds <= 60 * 1024
    return E, blocks


@pytest.mark.parametrize("case", LG.POINTER_FW, ids=LG.case_id)
def test_pointer_forward(case):
    B, nR, rows, Hd, S, _ = case
    E, blocks = _class_of(case, False)
    c = _Case(B, nR, rows, Hd, S, E, 31 * B + nR + S)
    shapes = ((nR,), (nR,), (Hd,))
    _lib.variant_hits_reset(DEV)
    full = [_canary(B + E, *s) for s in shapes]
    c.forward(0, B, full)
    assert len(c.launched(0)) == 1
    again = [_canary(B + E, *s) for s in shapes]
    c.forward(0, B, again)
    parts = [_canary(B, *s) for s in shapes]
    for lo, hi in c.chunks():
        assert c.geometry(hi - lo, False)[0] == 1
        c.forward(lo, hi, [o[lo:hi] for o in parts])
    torch.cuda.synchronize()
    for name, a, b, one in zip(("logits", "attn", "t"), full, again, parts):
        assert _untouched(a[B:]) and _written(a[:B]) and _written(one), name
        assert _differing_envs(a[:B], b[:B]) == [], name                               # two calls: the same bytes
        assert _differing_envs(a[:B], one) == [], (name, "E = %d against one env per workgroup" % E)
    want, e_ref = c.model_forward()
    at = torch.from_numpy(c.idx).to(DEV)
    got = [o[at].cpu().numpy() for o in full]
    worst = _held("geometry forward %s E %d" % (case[:5], E), list(zip(("logits", "attn", "t"), got, want, e_ref)))
    assert float((full[1][:B].sum(1) - 1).abs().max()) <= 1e-5                          # attn is a softmax over ALL columns
    print("geometry forward %s E %d (%d workgroups): worst err / e_ref %.2f" % (case[:5], E, blocks, worst))


@pytest.mark.parametrize("case", LG.POINTER_BW, ids=LG.case_id)
def test_pointer_backward(case):
    B, nR, rows, Hd, S, _ = case
    E, blocks = _class_of(case, True)
    c = _Case(B, nR, rows, Hd, S, E, 37 * B + nR + S)
    fwd = [torch.empty(B, *s, device=DEV) for s in ((nR,), (nR,), (Hd,))]
    c.forward(0, B, fwd)
    attn, t = fwd[1], fwd[2]
    pad = 64                                                                            # canary floats behind dva, dvp and the scratch
    shapes = ((B + E, 3 * Hd, nR), (B + E, Hd), (Hd + pad,), (Hd + pad,))
    words = blocks * 2 * Hd
    _lib.variant_hits_reset(DEV)
    full, scratch = [_canary(*s) for s in shapes], _canary(words + pad)
    assert c.backward(0, B, attn, t, full, scratch) == 4 * words
    assert len(c.launched(1)) == 1
    again = [_canary(*s) for s in shapes]
    c.backward(0, B, attn, t, again, _canary(words + pad))
    parts = [_canary(B, 3 * Hd, nR), _canary(B, Hd), _canary(Hd), _canary(Hd)]
    small = _canary(CHUNK * 2 * Hd)
    for lo, hi in c.chunks():
        assert c.geometry(hi - lo, True)[0] == 1
        c.backward(lo, hi, attn, t, [parts[0][lo:hi], parts[1][lo:hi], parts[2], parts[3]], small)
    torch.cuda.synchronize()
    assert _untouched(scratch[words:]) and _written(scratch[:words])
    for name, a, b in zip(("dU", "dq", "dva", "dvp"), full, again):
        n = B if name in ("dU", "dq") else Hd
        assert _untouched(a[n:]) and _written(a[:n]), name
        assert _i32(a[:n]).equal(_i32(b[:n])), name                                    # two calls: the same bytes
    for name, a, one in zip(("dU", "dq"), full, parts):
        assert _written(one) and _differing_envs(a[:B], one) == [], (name, "E = %d against one env per workgroup" % E)
    # the sample against the float64 model of those envs
    at = torch.from_numpy(c.idx).to(DEV)
    gs = c.grad[at].cpu().numpy()
    want, ref32 = (_autograd(S, c.small, c.X["dyn"], gs, d) for d in (torch.float64, torch.float32))
    label = "geometry backward %s E %d" % (case[:5], E)
    worst = _held(label, [(n, a[at].cpu().numpy(), want[n], ref32[n]) for n, a in zip(("dU", "dq"), full)])
    if nR == 4:
        worst = max(worst, _batch_sums(c, label, full))
    print("%s (%d workgroups): worst err / e_ref %.2f" % (label, blocks, worst))


def _batch_sums(c, label, raw):
    """dva, dvp, dM, dk (and dG, dg): the autograd function on the whole batch against float64 autograd of the folded model
    over the whole batch; the raw entry's dva / dvp are the function's bytes"""
    B, Hd, S = c.B, c.Hd, c.S
    params = [v.clone().requires_grad_(True) for v in ((c.G, c.g) if S else ()) + (c.M, c.k, c.va, c.vp)]
    if S:
        logits = T.pointer_scores_static(c.xs, c.bits, params[0], params[1], params[2], params[3], c.q, params[4], params[5], rows=c.rows)
        names = ("dG", "dg", "dM", "dk", "dva", "dvp")
    else:
        logits = T.pointer_scores(c.proj, c.bits, params[0], params[1], c.q, params[2], params[3], rows=c.rows)
        names = ("dM", "dk", "dva", "dvp")
    logits.backward(c.grad)
    got = {n: v.grad.cpu().numpy() for n, v in zip(names, params)}
    assert got["dva"].tobytes() == raw[2][:Hd].cpu().numpy().tobytes() and got["dvp"].tobytes() == raw[3][:Hd].cpu().numpy().tobytes()
    cpu = lambda v: v.cpu().numpy()
    if S:
        inp = (cpu(c.xs), cpu(c.G), cpu(c.g), cpu(c.M), cpu(c.k), cpu(c.q), cpu(c.va), cpu(c.vp))
    else:
        inp = (M.from_layout(cpu(c.proj)), cpu(c.M), cpu(c.k), cpu(c.q), cpu(c.va), cpu(c.vp))
    dyn, grad = cpu(c.dyn), cpu(c.grad)
    want, ref32 = (_autograd(S, inp, dyn, grad, d) for d in (torch.float64, torch.float32))
    return _held(label + " whole batch", [(n, got[n], want[n], ref32[n]) for n in names])


# ---- the encoder ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nR,rows,H", LG.ENCODER_FW)
def test_encoder_forward_is_the_models_bytes(B, nR, rows, H):
    epb, gx, gy, _ = _lib.encode_bits_geometry(B, nR, rows, H, False)
    assert epb > 2 and gx == -(-B // epb)
    for i, density in enumerate((0.05, 0.5)):
        dyn, bits, W, b = EM.random_case(B, rows, nR, H, density, 100 * rows + B + i)
        out = _canary(B + epb, H, nR)
        rollout._encode_into(_dev(bits), _dev(W), _dev(b), rows, out[:B])
        torch.cuda.synchronize()
        assert _untouched(out[B:])
        got, want = out[:B].cpu().numpy(), EM.encode(bits, W, b, rows, nR)
        assert np.array_equal(got, want), (density, np.argwhere(got != want)[:4])
    print("geometry encoder forward %s: %d envs per workgroup, grid (%d, %d)" % ((B, nR, rows, H), epb, gx, gy))


@pytest.mark.parametrize("B,nR,rows,H", LG.ENCODER_BW)
def test_encoder_backward(B, nR, rows, H):
    per, slices, chunks, hc = _lib.encode_bits_geometry(B, nR, rows, H, True)
    assert per > 3 and B % per
    dyn, bits, W, b = EM.random_case(B, rows, nR, H, 0.4, 50 + rows, spiky=False)
    g = np.random.RandomState(51 + rows).randn(B, H, nR).astype(np.float32)
    dW64, db64, dWm, dbm = EM.backward64(bits, g, rows, nR)
    K = B * nR                                                     # terms per element; the bound holds for ANY summation order
    L, c = _lib.lib(), _lib.ctx(torch.device(DEV))
    need = int(L.tap_encode_bits_backward_scratch(B, nR, rows, H))
    assert need == slices * H * (rows + 1) * 4
    tb, tg = _dev(bits), _dev(g)
    res = []
    for _ in range(2):
        scratch, dW, db = _canary(need // 4 + 64), _canary(H * rows + 64), _canary(H + 64)
        _lib.check(L.tap_encode_bits_backward(c, _lib.ptr(tb), _lib.ptr(tg), B, nR, rows, H, _lib.ptr(dW), _lib.ptr(db),
                                              _lib.ptr(scratch), need, _lib.stream_of(torch.device(DEV))), c)
        torch.cuda.synchronize()
        assert _untouched(scratch[need // 4:]) and _untouched(dW[H * rows:]) and _untouched(db[H:]) and _written(scratch[:need // 4])
        res.append((dW[:H * rows].view(H, rows).cpu().numpy(), db[:H].cpu().numpy()))
    (dW, db), (dW2, db2) = res
    eW, eb = np.abs(dW - dW64), np.abs(db - db64)
    print("geometry encoder backward %s: %d envs per slice, %d slices, %d chunks of %d; worst err / bound dW %.3g db %.3g"
          % ((B, nR, rows, H), per, slices, chunks, hc, (eW / np.maximum(K * EM.U32 * dWm, 1e-300)).max(), (eb / (K * EM.U32 * dbm)).max()))
    assert np.isfinite(dW).all() and np.isfinite(db).all() and np.abs(dW64).max() > 0
    assert (eW <= K * EM.U32 * dWm).all(), eW.max()
    assert (eb <= K * EM.U32 * dbm).all(), eb.max()
    assert dW.tobytes() == dW2.tobytes() and db.tobytes() == db2.tobytes()             # deterministic: the same bytes


# ---- the critic: the tests of test_critic_gpu.py at the large batches -------------------------------------------------
@pytest.mark.parametrize("rows,nR,H,S,n,B", LG.CRITIC_FW)
def test_critic_forward(rows, nR, H, S, n, B):
    import test_critic_gpu as CG
    CG.test_forward(rows, nR, H, S, n, B)


@pytest.mark.parametrize("rows,nR,H,S,n,B", LG.CRITIC_BW)
def test_critic_backward(rows, nR, H, S, n, B):
    import test_critic_gpu as CG
    blocks = int(_lib.lib().tap_critic_value_backward_scratch(B, nR, rows, H, S, n)) // (4 * H)
    assert blocks == -(-B // 4) and blocks > LG.REDUCE_RUN and B % 4
    CG.test_backward(rows, nR, H, S, n, B, False)
