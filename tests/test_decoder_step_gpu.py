"""The decoder step on the MI355X (decoder.hip: k_decoder_step, k_decoder_step_bw) against the float64 model of
tests/decoder_step_model.py.

The tolerance is the project's rule, pointer_model.tolerance, not a constant.  Per case the reference's own form (two
nn.Conv1d encoders, their concatenation, nn.GRU for one step, the decoder's columns of the attention's W -- model.py:347-354,
108-115) is evaluated in float32 torch on the CPU; its largest error against float64 is ``e_ref``, and the kernel must stay
within 4 e_ref + 16 * 2^-24 * max |want|.  The kernel's inputs are the float64 fold of the case rounded to float32, and
``want`` is the float64 model ON those rounded inputs, so no input rounding enters the comparison.  The reference's form
does not name the gates; their e_ref is the float32 run of the model's torch form on the same rounded inputs.  Each test
prints its worst err / e_ref."""
import copy

import numpy as np
import pytest
import torch

import decoder_step_model as M
import episode_actor_model as A
import pointer_model as PM
import tap_net_amd as T
from tap_net_amd import _lib, rollout, synth, tools
from test_episode_autograd_gpu import _against_the_float64_loop, _loss_backward, _to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TE = 16                                 # envs per workgroup (decoder.hip: DEC_TE)

# (Ks, Kd, Hd, B): c2's six raw decoder values at every Hd with a kernel; K below, at and above one block of 32 terms, with
# and without a ragged last four; each single encoder; Ks + Kd = Hd + 16 at the smallest and the largest Hd; one env, a
# ragged tile, many tiles with a full (2050 = 128 * 16 + 2) and an odd (2051) last one
CASES = [(2, 4, 64, 1), (2, 4, 128, 67), (3, 50, 128, 3), (0, 4, 64, 3), (3, 0, 256, 2), (3, 64, 128, 5), (3, 77, 64, 2),
         (16, 256, 256, 2), (2, 4, 64, 2050), (2, 4, 64, 2051)]
BW_CASES = [(2, 4, 128, 67), (3, 64, 64, 3), (3, 0, 256, 2), (2, 4, 64, 2051)]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)


def _keys(extra):
    return {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_DECODER and k[5] == extra}


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))


_made = {}


def _inputs(Ks, Kd, Hd, B):
    """-> X (the reference form's inputs) and the kernel's float32 inputs (xs, xd, h, P, c, w_hh, b_hh, wq), made once per
    case and left unchanged"""
    key = (Ks, Kd, Hd, B)
    if key not in _made:
        X = M.make_case(B, Ks, Kd, Hd, 1000 * Ks + 10 * Kd + Hd + B)
        P, c = (np.asarray(a, np.float32) for a in M.fold(X, np.float64))
        _made[key] = (X, (X["xs"], X["xd"], X["h"], P, c, X["W_hh"], X["b_hh"], X["Wq"]))
    return _made[key]


def _raw(inp, with_h=True, want_gates=True):
    """the forward entry on device copies -> h', q, gates (None when not asked for) as numpy"""
    xs, xd, h, P, c, w_hh, b_hh, wq = inp
    B, Hd = xs.shape[0], wq.shape[0]
    hn, q = (torch.full((B, Hd), float('nan'), device=DEV) for _ in range(2))
    gates = torch.full((B, 4, Hd), float('nan'), device=DEV) if want_gates else None
    rollout._decoder_into(_dev(xs) if xs.shape[1] else None, _dev(xd) if xd.shape[1] else None, _dev(h) if with_h else None,
                          _dev(P), _dev(c), _dev(w_hh), _dev(b_hh), _dev(wq), hn, q, gates)
    return [hn.cpu().numpy(), q.cpu().numpy(), None if gates is None else gates.cpu().numpy()]


@pytest.mark.parametrize("Ks,Kd,Hd,B", CASES)
def test_forward(Ks, Kd, Hd, B):
    X, inp = _inputs(Ks, Kd, Hd, B)
    worst = 0.0
    for with_h in (True, False):
        mine = inp[:2] + (inp[2] if with_h else None,) + inp[3:]
        want = M.step(*mine)
        with torch.no_grad():
            r32, r64 = (M.reference_form_torch(X, d, with_h) for d in (torch.float32, torch.float64))
            g32, g64 = (M.step_torch(*(_t(a, d) for a in mine))[2] for d in (torch.float32, torch.float64))
        e_ref = [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)] + [float((g32.double() - g64).abs().max())]
        _lib.variant_hits_reset(DEV)
        got = _raw(inp, with_h)
        assert _keys(0) == {(_lib.TAP_HIT_DECODER, 0, TE, Hd // 64, int(with_h), 0, 0)}, _keys(0)
        for name, g, w, e in zip(("h_new", "q", "gates"), got, want, e_ref):
            assert g.dtype == np.float32 and g.shape == w.shape and np.isfinite(g).all(), name
            err = float(np.abs(g.astype(np.float64) - w).max())
            print("decoder forward %s h %d %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
                  % ((Ks, Kd, Hd, B), with_h, name, err, e, _ratio(err, e), np.abs(w).max()))
            assert np.abs(w).max() > 0 and err <= PM.tolerance(e, w), (name, with_h, err, e)
            worst = max(worst, _ratio(err, e))
        # two calls give the same bytes; without gates_out h' and q are the same bytes
        again, bare = _raw(inp, with_h), _raw(inp, with_h, want_gates=False)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes()
        assert bare[2] is None and got[0].tobytes() == bare[0].tobytes() and got[1].tobytes() == bare[1].tobytes()
        if not with_h:
            # the zero state: gh is exactly b_hh, and w_hh does not enter, whatever it holds
            other = _raw(inp[:5] + (np.full_like(inp[5], 1e30),) + inp[6:], False)
            for a, b in zip(got, other):
                assert a.tobytes() == b.tobytes()
            assert np.array_equal(got[2][:, 3], np.broadcast_to(inp[6][2 * Hd:], (B, Hd)))
        if B > TE:
            # an env's bytes do not depend on the batch around it: the last env alone
            alone = _raw(tuple(a[-1:] for a in inp[:3]) + inp[3:], with_h)
            for a, b in zip(got, alone):
                assert a[-1:].tobytes() == b.tobytes()
    print("decoder forward %s: worst err / e_ref %.2f" % ((Ks, Kd, Hd, B), worst))


def test_launch_record_names_the_instantiation():
    seen = set()
    for Hd in (64, 128, 256):
        for with_h in (True, False):
            _lib.variant_hits_reset(DEV)
            z = lambda *s: torch.zeros(*s, device=DEV)
            with torch.no_grad():
                hn, q = T.decoder_step(z(3, 2, 1), z(3, 4, 1), z(3, Hd) if with_h else None, z(3 * Hd, 6), z(3 * Hd), z(3 * Hd, Hd),
                                       z(3 * Hd), z(Hd, Hd))
            assert tuple(hn.shape) == tuple(q.shape) == (3, Hd) and not bool(hn.any()) and not bool(q.any())
            assert _keys(0) == {(_lib.TAP_HIT_DECODER, 0, TE, Hd // 64, int(with_h), 0, 0)} and not _keys(1)
            seen |= _keys(0)
    assert len(seen) == 6
    assert {c[2] for c in CASES} == {64, 128, 256} and any(c[3] > TE and c[3] % TE for c in CASES)
    assert {(c[0] + c[1]) for c in CASES} >= {6, 53, 67, 80, 272} and any(c[0] + c[1] == c[2] + 16 for c in CASES)


def test_statuses_in_the_headers_order():
    L, c = _lib.lib(), _lib.ctx(DEV)
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED
    B, Hd = 2, 64
    buf = torch.zeros(8 * 3 * 96 * 96 + 16, device=DEV)              # one zeroed buffer serves as every input,
    outs = torch.zeros(3, 4096, device=DEV)                           # three others as the outputs (B * 4 * Hd = 512 floats at most)
    p, po = _lib.ptr(buf), [_lib.ptr(outs[i]) for i in range(3)]
    off = _lib._vp(buf.data_ptr() + 2)
    st = _lib.stream_of(torch.device(DEV))

    def fwd(B, Ks, Kd, Hd, bufs):
        return L.tap_decoder_step(c, bufs[0], Ks, bufs[1], Kd, bufs[2], B, Hd, *bufs[3:11], st)

    def bwd(B, Hd, bufs):
        return L.tap_decoder_step_backward(c, B, Hd, *bufs, st)
    every, none = [p] * 8 + po, [None] * 11
    assert fwd(-1, 2, 4, Hd, every) == inv and fwd(B, -1, 4, Hd, every) == inv and fwd(B, 2, -1, Hd, every) == inv
    assert fwd(B, 2, 4, 0, every) == inv and fwd(0, 2, 4, -1, none) == inv
    assert fwd(0, 2, 4, Hd, none) == ok and fwd(0, 2, 4, 96, none) == ok and fwd(0, 0, 0, Hd, none) == ok
    for hole in range(11):
        args = list(every)
        args[hole] = None
        for dims in ((2, 4, Hd), (2, 4, 96)):                         # a null buffer comes before the shape
            want = inv if hole not in (2, 10) else (ok if dims[2] == Hd else uns)
            assert fwd(B, *dims, args) == want, (hole, dims)
    assert fwd(B, 0, 4, Hd, [None] + every[1:]) == ok and fwd(B, 2, 0, Hd, [p, None] + every[2:]) == ok
    for dims in ((2, 4, 96), (2, 4, 32), (0, 0, Hd), (4, Hd + 13, Hd), (Hd + 17, 0, Hd)):
        assert fwd(B, *dims, every) == uns, dims
    assert fwd(B, 4, Hd + 12, Hd, every) == ok                        # Ks + Kd = Hd + 16
    for hole in range(11):
        args = list(every)
        args[hole] = off
        assert fwd(B, 2, 4, Hd, args) == inv, hole
    with pytest.raises(T.TapError) as ei:
        z = lambda *s: torch.zeros(*s, device=DEV)
        rollout._decoder_into(z(B, 2), z(B, 4), None, z(3 * 96, 6), z(3 * 96), z(3 * 96, 96), z(3 * 96), z(96, 96), z(B, 96), z(B, 96), None)
    assert ei.value.status == uns and "Hd 96" in str(ei.value)
    six = [p] * 3 + po
    assert bwd(-1, Hd, six) == inv and bwd(B, 0, six) == inv and bwd(0, Hd, [None] * 6) == ok and bwd(0, 96, [None] * 6) == ok
    for hole in range(6):
        args = list(six)
        args[hole] = None
        assert bwd(B, Hd, args) == (ok if hole == 1 else inv) and bwd(B, 96, args) == (uns if hole == 1 else inv), hole
        args[hole] = off
        assert bwd(B, Hd, args) == inv, hole
    assert bwd(B, 96, six) == uns and bwd(B, Hd, six) == ok
    torch.cuda.synchronize()


def _grads_torch(inp, with_h, xd_grad, g, dtype):
    """autograd of the model in torch on the CPU -> {name: gradient} of L = sum(h' g[0]) + sum(q g[1])"""
    names = ("xs", "xd", "h", "P", "c", "w_hh", "b_hh", "wq")
    leaves = dict(zip(names, (_t(a, dtype) for a in inp)))
    if not with_h:
        leaves["h"] = None
    wanted = [n for n in names[3:] + (("h",) if with_h else ()) + (("xd",) if xd_grad else ())]
    for n in wanted:
        leaves[n].requires_grad_(True)
    hn, q, _ = M.step_torch(*(leaves[n] for n in names))
    ((hn * _t(g[0], dtype)).sum() + (q * _t(g[1], dtype)).sum()).backward()
    return {n: (torch.zeros_like(leaves[n]) if leaves[n].grad is None else leaves[n].grad).double().numpy() for n in wanted}   # (no h: w_hh is unused)


def _grads_device(inp, with_h, xd_grad, g):
    names = ("xs", "xd", "h", "P", "c", "w_hh", "b_hh", "wq")
    leaves = dict(zip(names, (_dev(a) for a in inp)))
    if not with_h:
        leaves["h"] = None
    if not inp[0].shape[1]:
        leaves["xs"] = None
    if not inp[1].shape[1]:
        leaves["xd"] = None
    wanted = [n for n in names[3:] + (("h",) if with_h else ()) + (("xd",) if xd_grad else ())]
    for n in wanted:
        leaves[n].requires_grad_(True)
    hn, q = T.decoder_step(*(leaves[n] for n in names))
    assert hn.requires_grad and q.requires_grad
    ((hn * _dev(g[0])).sum() + (q * _dev(g[1])).sum()).backward()
    return {n: leaves[n].grad.double().cpu().numpy() for n in wanted}


@pytest.mark.parametrize("Ks,Kd,Hd,B", BW_CASES)
def test_backward(Ks, Kd, Hd, B):
    """the gradients of P, c, w_hh, b_hh, wq and h -- and of xd where it requires grad, the encoded dynamic half of the 3D
    case -- through rollout.decoder_step, against float64 autograd of the model; e_ref from its float32 CPU autograd"""
    X, inp = _inputs(Ks, Kd, Hd, B)
    rng = np.random.RandomState(Ks + Kd + B)
    g = rng.randn(2, B, Hd).astype(np.float32)
    xd_grad = Kd == 64
    worst = 0.0
    for with_h in ((True, False) if B == 67 else (True,)):
        want = _grads_torch(inp, with_h, xd_grad, g, torch.float64)
        ref32 = _grads_torch(inp, with_h, xd_grad, g, torch.float32)
        _lib.variant_hits_reset(DEV)
        got = _grads_device(inp, with_h, xd_grad, g)
        assert _keys(1) == {(_lib.TAP_HIT_DECODER, 0, TE, Hd // 64, int(with_h), 1, 0)}, _keys(1)
        assert sorted(got) == sorted(want) and len(got) == 5 + int(with_h) + int(xd_grad)
        for name in sorted(want):
            a, w, r = got[name], want[name], ref32[name]
            assert a.shape == w.shape and np.isfinite(a).all(), name
            e, err = float(np.abs(r - w).max()), float(np.abs(a - w).max())
            print("decoder backward %s h %d %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
                  % ((Ks, Kd, Hd, B), with_h, name, err, e, _ratio(err, e), np.abs(w).max()))
            if name == "w_hh" and not with_h:
                assert not a.any() and not w.any()                    # the zero state: w_hh did not enter
                continue
            assert np.abs(w).max() > 0 and err <= PM.tolerance(e, w), (name, with_h, err, e)
            worst = max(worst, _ratio(err, e))
    print("decoder backward %s: worst err / e_ref %.2f" % ((Ks, Kd, Hd, B), worst))


def test_backward_launch_gives_the_same_bytes_twice():
    """the launch's own outputs against the model's element-wise formulas in float64, and byte for byte on a second call"""
    B, Hd = 2051, 64
    X, inp = _inputs(2, 4, Hd, B)
    _, _, gates = _raw(inp)
    g = np.random.RandomState(5).randn(B, Hd).astype(np.float32)
    for with_h in (True, False):
        outs = []
        for _ in range(2):
            o = [torch.full(s, float('nan'), device=DEV) for s in ((B, 3 * Hd), (B, Hd), (B, Hd))]
            rollout._decoder_backward_into(_dev(gates), _dev(inp[2]) if with_h else None, _dev(g), *o)
            outs.append([v.cpu().numpy() for v in o])
        for a, b in zip(*outs):
            assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
        r, z, n, ghn = (gates[:, i].astype(np.float64) for i in range(4))
        h, g64 = (inp[2].astype(np.float64) if with_h else 0.0), g.astype(np.float64)
        dan = g64 * (1 - z) * (1 - n * n)
        want = [np.concatenate((dan * ghn * r * (1 - r), g64 * (h - n) * z * (1 - z), dan), axis=1), dan * r, g64 * z]
        # every output is g times factors of at most 1 (h - n: 2) and, for da_r, gh_n; at most 8 roundings, each 2^-24 of that
        bound = 16 * PM.U32 * float(np.abs(g64).max()) * max(1.0, float(np.abs(ghn).max()))
        for a, w in zip(outs[0], want):
            assert np.abs(w).max() > 0 and float(np.abs(a - w).max()) <= bound


# ---- through the modules -----------------------------------------------------------------------------------------------
def _setup(D, B, seed):
    """B instances of the 2D c2 window (n = 10: rows 30, nR 20; K = 2 + 4) or of the two-plane 3D window (n = 22: rows 66,
    nR 132; K = 3 + 50), the actor of tests/episode_actor_model.py (H = 64, the decoder's two encodings summed), and the
    pre-drawn u (n, B), adv (B,) and ghh (1, B, H)"""
    n = 10 if D == 2 else 22
    cs = [5, 50] if D == 2 else [5, 5, 200]
    static, dynamic = synth.rand_instances(B, n, D, seed=seed)
    rng = np.random.RandomState(seed + 1)
    u = rng.rand(n, B).astype(np.float32)
    adv = rng.randn(B).astype(np.float32)
    ghh = rng.randn(1, B, A.H).astype(np.float32)
    flen = (cs[0] - 1) if D == 2 else 2 * cs[0] * cs[1]
    return dict(B=B, n=n, D=D, cs=cs, static=static, dynamic=dynamic, u=u, adv=adv, ghh=ghh,
                actor=A.make_actor(static, dynamic, flen, seed + 2))


def _step_path(S):
    """a lean stepper, proj and the two folds once per episode, forward_step + the head per step, one backward()"""
    net = copy.deepcopy(S["actor"]).to(DEV).train()
    static, dynamic, u = S["static"].to(DEV).contiguous(), S["dynamic"].to(DEV).contiguous(), _to(S["u"])
    env = T.BatchedContainer(S["B"], S["cs"], S["n"], "C+P+S-lb-soft", "diff", device=DEV)
    state = {}

    def scorer(step, decoder_static, decoder_dynamic, **_):
        logits, state["hh"] = net.pointer.forward_step(state["proj"], sp.dynamic_bits, state["fold"], decoder_static, decoder_dynamic,
                                                       state["hh"])
        return logits
    _lib.variant_hits_reset(DEV)
    with torch.enable_grad():
        sp = T.EpisodeStepper(static, dynamic, env, expand_dynamic=False)
        state["proj"] = net.pointer.project_static(net.static_encoder(static))
        P, c = net.pointer.fold_decoder(net.decoder_static_encoder, net.decoder_dynamic_encoder, combine='sum')
        state["fold"] = net.pointer.fold_episode(net.dynamic_encoder, P, c)
        state["hh"] = None
        pol = T.PointerHeadPolicy(scorer, u=u)
        out = T.run_episode(static, dynamic, pol, S["cs"][0], S["cs"][-1], stepper=sp, check=False)
        tour_logp = pol.tour_logp()
        _loss_backward(S, tour_logp, state["hh"])
    sp.check()
    hits = {(kind, extra): sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == kind and k[5] == extra)
            for kind in (_lib.TAP_HIT_DECODER, _lib.TAP_HIT_POINTER) for extra in (0, 1)}
    assert set(hits.values()) == {S["n"]}, hits                       # both kernels ran: n forward and n backward launches each
    return out["tour_idx"].cpu().numpy(), tour_logp.detach().double().cpu().numpy(), A.named_grads(net)


@pytest.mark.parametrize("D,B", [(2, 67), (3, 3)])
def test_training_step_through_forward_step(D, B):
    """fold_decoder + fold_episode + forward_step on EpisodeStepper(expand_dynamic=False), teacher-forced through
    episode_actor_model.train_step in float64 (wanted) and float32 (e_ref): tour_logp and the gradient of every parameter,
    the two decoder encoders and pointer.gru.* included"""
    S = _setup(D, B, 41 if D == 2 else 63)
    assert tuple(S["dynamic"].shape) == ((B, 30, 20) if D == 2 else (B, 66, 132))
    _against_the_float64_loop("step path %dD" % D, S, *_step_path(S))


def test_forward_step_equals_forward_bits_on_the_device():
    """the two launches against today's path (decoder convolutions + forward_bits) on the same device tensors, eval mode:
    within the sum of both paths' tolerances is not needed -- both are float32 paths of the same function, so the float64
    CPU run of ``forward`` is the judge and e_ref its float32 run"""
    B, rows, nR, H = 5, 30, 20, 128
    torch.manual_seed(51)
    net = tools.Pointer(H, H, 'shape_heightmap', 'bot').eval()
    for p in net.parameters():
        torch.nn.init.xavier_uniform_(p) if p.dim() > 1 else torch.nn.init.normal_(p, std=0.1)
    enc = T.DynamicBitsEncoder(rows, H)
    dec_s, dec_d = torch.nn.Conv1d(2, H // 2, 1), torch.nn.Conv1d(4, H // 2, 1)
    dyn = np.random.RandomState(52).rand(B, rows, nR) < 0.1
    sh, hh = torch.randn(B, H, nR), torch.tanh(torch.randn(1, B, H))
    ds, dd = torch.randint(0, 6, (B, 2, 1)).float(), torch.randint(0, 51, (B, 4, 1)).float()

    def float_path(dtype):
        mods = [copy.deepcopy(m).to(dtype) for m in (net, enc, dec_s, dec_d)]
        with torch.no_grad():
            hidden = torch.cat((mods[2](ds.to(dtype)), mods[3](dd.to(dtype))), 1)
            logits, last = mods[0](sh.to(dtype), mods[1](torch.from_numpy(dyn).to(dtype)), hidden, hh.to(dtype))
        return logits.double().numpy(), last.double().numpy()
    want, ref32 = float_path(torch.float64), float_path(torch.float32)
    n3, e3, s3, d3 = (copy.deepcopy(m).to(DEV) for m in (net, enc, dec_s, dec_d))
    bits = _dev(PM.pack_bits(dyn))
    _lib.variant_hits_reset(DEV)
    with torch.no_grad():
        proj = n3.project_static(sh.to(DEV))
        fold = n3.fold_episode(e3, *n3.fold_decoder(s3, d3))
        got = n3.forward_step(proj, bits, fold, ds.to(DEV), dd.to(DEV), hh.to(DEV))
        first = n3.forward_step(proj, bits, fold, ds.to(DEV), dd.to(DEV), None)
        zero = n3.forward_step(proj, bits, fold, ds.to(DEV), dd.to(DEV), torch.zeros(1, B, H, device=DEV))
    assert len(_keys(0)) == 2 and tuple(got[1].shape) == (1, B, H)
    for name, a, w, r in (("logits", got[0], want[0], ref32[0]), ("last_hh", got[1], want[1], ref32[1])):
        e, err = float(np.abs(r - w).max()), float(np.abs(a.double().cpu().numpy() - w).max())
        print("forward_step %s: err %.3g e_ref %.3g ratio %.2f" % (name, err, e, _ratio(err, e)))
        assert err <= PM.tolerance(e, w), (name, err, e)
    # None is the zero state: a zero h adds exact zeros to b_hh, term by term
    assert torch.equal(first[0], zero[0]) and torch.equal(first[1], zero[1])
    # training mode with the default dropout takes the torch path: no decoder launch
    _lib.variant_hits_reset(DEV)
    n3.train()
    with torch.no_grad():
        out = n3.forward_step(proj, bits, fold, ds.to(DEV), dd.to(DEV), hh.to(DEV))
    assert not _keys(0) and tuple(out[0].shape) == (B, nR)


def test_step_and_head_replay_from_a_hip_graph():
    B, rows, nR, H = 64, 30, 20, 128
    torch.manual_seed(61)
    net = tools.Pointer(H, H, 'shape_heightmap', 'bot').eval()
    for p in net.parameters():
        torch.nn.init.xavier_uniform_(p) if p.dim() > 1 else torch.nn.init.normal_(p, std=0.1)
    net = net.to(DEV)
    enc = T.DynamicBitsEncoder(rows, H).to(DEV)
    dec_s, dec_d = torch.nn.Conv1d(2, H // 2, 1).to(DEV), torch.nn.Conv1d(4, H // 2, 1).to(DEV)
    rng = np.random.RandomState(62)
    bits = _dev(PM.pack_bits(rng.rand(B, rows, nR) < 0.1))
    mask = _dev((rng.rand(B, nR) < 0.5).astype(np.float32))
    mask[:, 0] = 1
    u = _dev(rng.rand(B).astype(np.float32))
    sh, hh = torch.randn(B, H, nR, device=DEV), torch.tanh(torch.randn(1, B, H, device=DEV))
    ds, dd = torch.randint(0, 6, (B, 2, 1), device=DEV).float(), torch.randint(0, 51, (B, 4, 1), device=DEV).float()

    def step():
        logits, last = net.forward_step(proj, bits, fold, ds, dd, hh)
        ptr, logp = T.pointer_pick(logits, mask, u)
        return logits, last, ptr, logp
    with torch.no_grad():
        proj = net.project_static(sh)
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
        eager = step()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = step()
        for _ in range(2):
            for v in rec:
                v.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(rec, eager):
                assert torch.equal(a, b)
    assert bool(torch.isfinite(eager[0]).all()) and float(eager[0].abs().max()) > 0 and bool(torch.isfinite(eager[3]).all())
