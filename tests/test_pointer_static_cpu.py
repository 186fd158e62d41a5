"""The pointer network's static-rows form without a GPU: the float64 fold against the reference's form
(tests/pointer_static_model.py), ``Pointer.fold_static`` and the ``StaticFold`` record through ``forward_bits``, ``forward_step``
and their ``_dropout`` forms in float64 -- off the GPU the record's torch path is ``forward`` on ``static_encoder(xs)``, so the
module is its own model --, the reference's recorded actor through the record, and the wrapper's argument errors.

Every bound is 1e-12 * max |want| (DESIGN 7i's bound for folds): float64 arithmetic in another order, sums of a few hundred
terms of O(1), not a measurement."""
import copy
import ctypes as C
import inspect

import numpy as np
import pytest
import torch
from torch import nn

import actor_reference_cases as AC
import oracle_lib as O
import pointer_model as M
import pointer_static_model as SM
import tap_net_amd as T
from tap_net_amd import _lib, tools

BOUND = 1e-12


def _close(name, got, want, bound=BOUND, zero_ok=False):
    got, want = (np.asarray(a.detach().numpy() if torch.is_tensor(a) else a, np.float64) for a in (got, want))
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert got.shape == want.shape and (top > 0 or zero_ok) and err <= bound * top, (name, err, top)


def test_static_fold_equals_the_reference_form():
    for rows, nR, He, Hd, S in ((30, 20, 128, 128, 2), (126, 60, 64, 128, 3), (10, 4, 128, 64, 8), (30, 20, 32, 64, 1)):
        X = SM.make_case(3, rows, nR, He, Hd, S, 0.1, 13 * rows + nR + S)
        want = M.reference_form(X, np.float64)
        G, g, Mf, k, q = SM.fold(X, np.float64)
        assert G.shape == (3 * Hd, S) and g.shape == (3 * Hd,)
        P = SM.static_term(X["xs"], G, g, np.float64)
        _close("P", P, M.fold(X, np.float64)[0])
        got = M.folded(P, X["dyn"], Mf, k, q, X["va"], X["vp"], np.float64)
        for name, a, w in zip(("logits", "attn", "t"), got, want):
            _close(name, a, w)
        assert np.abs(want[0]).max() > 0.1
        c = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        tt = SM.folded_torch(c(X["xs"]), c(G), c(g), c(X["dyn"]), c(Mf), c(k), c(q), c(X["va"]), c(X["vp"]))
        rt = SM.reference_form_torch(X, torch.float64)
        for name, a, b, w in zip(("logits", "attn", "t"), tt, rt, want):
            _close(name + " (torch, folded)", a, w)
            _close(name + " (torch, reference)", b, w)


# ---- the modules ---------------------------------------------------------------------------------------------------------
HE, HD, B_, ROWS, NR, S_ = 32, 64, 5, 30, 20, 3        # a shape WITH a kernel: off the GPU the record still takes the torch path


def _mods(seed=5, p=0.0):
    torch.manual_seed(seed)
    net = tools.Pointer(HE, HD, 'shape_heightmap', 'bot', dropout=p).double()
    for q in net.parameters():
        nn.init.xavier_uniform_(q) if q.dim() > 1 else nn.init.normal_(q, std=0.1)
    enc = T.DynamicBitsEncoder(ROWS, HE).double()
    senc = nn.Conv1d(S_, HE, 1).double()
    dec_s, dec_d = nn.Conv1d(2, HD // 2, 1).double(), nn.Conv1d(4, HD // 2, 1).double()
    return net, enc, senc, dec_s, dec_d


def _inputs(seed=6, rows=ROWS, nR=NR):
    g = torch.Generator().manual_seed(seed)
    xs = torch.randint(1, 9, (B_, S_, nR), generator=g).double()
    dyn = (torch.rand(B_, rows, nR, generator=g) < 0.3).double()
    ds = torch.randint(0, 6, (B_, 2, 1), generator=g).double()
    dd = torch.randint(0, 51, (B_, 4, 1), generator=g).double()
    hh = torch.tanh(torch.randn(1, B_, HD, generator=g)).double()
    gl, gh = torch.randn(B_, nR, generator=g).double(), torch.randn(1, B_, HD, generator=g).double()
    return xs, dyn, ds, dd, hh, gl, gh


def _grads(mods):
    return {"%d.%s" % (i, n): p.grad for i, m in enumerate(mods) for n, p in m.named_parameters()}


def test_fold_static_is_project_static_of_the_encoders_output():
    """the record's fields, and g + G . xs against project_static(static_encoder(xs)): values and, through a random
    cotangent, the gradients of the encoder's and the two W's parameters"""
    mods = _mods()
    xs = _inputs()[0]
    r = torch.randn(B_, 3, NR, HD, generator=torch.Generator().manual_seed(3)).double()

    def run(ms, static):
        net, senc = ms[0], ms[2]
        if static:
            sf = net.fold_static(senc, xs)
            proj = (sf.g[None, :, None] + torch.einsum('xs,bsc->bxc', sf.G, sf.xs)).view(B_, 3, HD, NR).transpose(2, 3)
        else:
            proj = net.project_static(senc(xs))
        (proj * r).sum().backward()
        return proj.detach(), _grads(ms)
    got, want = run(copy.deepcopy(mods), True), run(copy.deepcopy(mods), False)
    _close("proj", got[0], want[0])
    for n in ("0.W", "0.encoder_attn.W", "2.weight", "2.bias"):
        _close(n, got[1][n], want[1][n])
    net, _, senc = mods[:3]
    wide = torch.zeros(B_, S_ + 1, NR).double()
    wide[:, 1:] = xs
    sf = net.fold_static(senc, wide[:, 1:, :])                       # the reference's static[:, 1:, :]: a non-contiguous slice
    assert isinstance(sf, T.StaticFold) and sf.static_encoder is senc and (sf.S, sf.nR) == (S_, NR)
    assert sf.xs.is_contiguous() and not sf.xs.requires_grad and torch.equal(sf.xs, xs)
    assert tuple(sf.G.shape) == (3 * HD, S_) and tuple(sf.g.shape) == (3 * HD,) and sf.G.requires_grad and sf.g.requires_grad

    class Wrapped(nn.Module):                                        # the reference's Encoder: its only layer is ``conv``
        def __init__(self):
            super(Wrapped, self).__init__()
            self.conv = senc

        def forward(self, x):
            return self.conv(x)
    assert torch.equal(net.fold_static(Wrapped(), xs).G, sf.G)
    for bad in (xs[:, :2], xs[0], xs.long()):
        with pytest.raises(ValueError):
            net.fold_static(senc, bad)
    with pytest.raises(ValueError):
        net.fold_static(nn.Conv1d(S_, HE, 3).double(), xs)
    assert len(list(net.parameters())) == 8                          # no parameter added: a reference checkpoint loads strictly


@pytest.mark.parametrize("form", ["bits", "step"])
def test_the_record_is_forward_on_the_static_encoders_output(form):
    """values and the gradient of every parameter, static_encoder's weight and bias included; with last_hh and without"""
    mods = _mods()
    xs, dyn, ds, dd, hh, gl, gh = _inputs()

    def run(ms, static, last):
        net, enc, senc, dec_s, dec_d = ms
        net.eval()
        hidden = torch.cat((dec_s(ds), dec_d(dd)), 1)
        if not static:
            logits, out = net(senc(xs), enc(dyn), hidden, last)
        elif form == "bits":
            logits, out = net.forward_bits(net.fold_static(senc, xs), dyn, enc, hidden, last)
        else:
            fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
            logits, out = net.forward_step(net.fold_static(senc, xs), dyn, fold, ds, dd, last)
        ((logits * gl).sum() + (out * gh).sum()).backward()
        return logits.detach(), out.detach(), _grads(ms)
    for last in (hh, None):
        got, want = run(copy.deepcopy(mods), True, last), run(copy.deepcopy(mods), False, last)
        assert got[0].dtype is torch.float64 and tuple(got[0].shape) == (B_, NR) and tuple(got[1].shape) == (1, B_, HD)
        _close("logits", got[0], want[0])
        _close("last_hh", got[1], want[1])
        assert sorted(got[2]) == sorted(want[2]) and len(got[2]) == 8 + 2 + 2 + 2 + 2
        for n in sorted(want[2]):
            assert got[2][n] is not None and want[2][n] is not None, n
            # (without a last_hh the GRU's hidden state is zero, and so is the gradient of weight_hh)
            _close(n, got[2][n], want[2][n], zero_ok=last is None and n == "0.gru.weight_hh_l0")


def test_a_packed_shadow_off_the_gpu_is_unpacked():
    """the record's torch path takes the int64 shadow too: the same bytes as the floating ``dynamic``, one and two planes"""
    for rows in (30, 70):
        net, _, senc, dec_s, dec_d = _mods()
        enc = T.DynamicBitsEncoder(rows, HE).double()
        xs, dyn, ds, dd, hh, _, _ = _inputs(rows=rows)
        bits = torch.from_numpy(M.pack_bits(dyn.numpy() != 0).view(np.int64))
        with torch.no_grad():
            sf = net.eval().fold_static(senc, xs)
            hidden = torch.cat((dec_s(ds), dec_d(dd)), 1)
            want = net.forward_bits(sf, dyn, enc, hidden, hh)
            got = net.forward_bits(sf, bits, enc, hidden, hh)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_dropout_forms_equal_their_proj_twins_under_the_same_masks():
    """train() with a StepDropout: two sources of one seed draw the same masks, so the record's forms and the ``proj`` forms
    are the same function.  rows 10 x nR 10 has no bit shadow, so the ``proj`` twin has a route off the GPU as well"""
    rows, nR = 10, 10
    net, _, senc, dec_s, dec_d = _mods(p=0.2)
    net.drop_rnn.p, net.drop_hh.p = 0.1, 0.3
    net.train()
    enc = T.DynamicBitsEncoder(rows, HE).double()
    xs, dyn, ds, dd, hh, _, _ = _inputs(rows=rows, nR=nR)
    a, b = T.StepDropout(31, "cpu", env_offset=2), T.StepDropout(31, "cpu", env_offset=2)
    with torch.no_grad():
        sf, proj = net.fold_static(senc, xs), net.project_static(senc(xs))
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
        hidden = torch.cat((dec_s(ds), dec_d(dd)), 1)
        s0 = torch.random.get_rng_state()
        for t, last in enumerate((hh, None)):
            got, want = net.forward_step_dropout(sf, dyn, fold, ds, dd, last, a), net.forward_step_dropout(proj, dyn, fold, ds, dd, last, b)
            assert a.step == b.step == 2 * t + 1
            _close("step logits %d" % t, got[0], want[0])
            _close("step last_hh %d" % t, got[1], want[1])
            assert bool((got[1] == 0).any()) and torch.equal(got[1] == 0, want[1] == 0)          # the same elements dropped
            got, want = net.forward_bits_dropout(sf, dyn, enc, hidden, last, a), net.forward_bits_dropout(proj, dyn, enc, hidden, last, b)
            _close("bits logits %d" % t, got[0], want[0])
            _close("bits last_hh %d" % t, got[1], want[1])
        assert torch.equal(s0, torch.random.get_rng_state())                                   # torch's generator was never touched
        net.eval()
        step = a.step
        want = net.forward_step(sf, dyn, fold, ds, dd, hh)
        got = net.forward_step_dropout(sf, dyn, fold, ds, dd, hh, a)
        assert a.step == step and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("D,ws", AC.CASES)
def test_the_references_actor_through_the_record(D, ws):
    """INTEGRATION 2i / 2j's recipe with fold_static in place of project_static, float64 on the CPU, teacher-forced on the
    recorded tour with grad enabled: per-step logits and last_hh, tour_logp, and after ONE backward() of
    L = sum_b adv[b] sum_t tour_logp[b, t] the gradient of every key of the reference's state dict"""
    z = AC.load(D, ws)
    mods, _ = AC.build(z, D)
    for m in mods.values():
        m.double()
    st, dyn = AC.instances(D)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    tour = z["tour_idx"].astype(np.int64)
    B, n, R = AC.BATCH[D], AC.N, st.shape[2] // AC.N
    dec_s, dec_d, enc, pointer = mods["static_decoder.conv."], AC.dynamic_decoder(mods), mods["dynamic_encoder."], mods["pointer."]
    sf = pointer.fold_static(mods["static_encoder.conv."], t64(st)[:, 1:, :])
    assert (sf.S, sf.nR) == (D, st.shape[2])
    fold = pointer.fold_episode(enc, *pointer.fold_decoder(dec_s, dec_d, combine='cat'))
    cur, mask = O.initial_mask(dyn, n), np.ones((B, st.shape[2]), np.float32)
    hh, logps = None, []
    for k in range(n):
        assert np.array_equal(cur, z["current_mask"][k].astype(np.float32)), k
        logits, hh = pointer.forward_step(sf, t64(dyn), fold, t64(z["decoder_static"][k]), t64(z["decoder_dynamic"][k]), hh)
        assert logits.dtype is torch.float64 and logits.requires_grad and tuple(hh.shape) == (1, B, AC.HD)
        _close("logits %d" % k, logits, z["logits"][k])
        _close("last_hh %d" % k, hh[0], z["last_hh"][k])
        logps.append(torch.log_softmax(logits + torch.log(t64(cur)), dim=1).gather(1, torch.from_numpy(tour[:, k:k + 1]))[:, 0])
        dyn = O.update_dynamic(dyn, st, tour[:, k], n, 3)
        cur, mask = O.update_mask(mask, dyn, tour[:, k], n, R)
    assert not mask.any()
    tour_logp = torch.stack(logps, dim=1)
    err = float((tour_logp.detach() - t64(z["tour_logp"])).abs().max())
    assert err <= BOUND * max(1.0, float(np.abs(z["tour_logp"]).max())), err
    (t64(z["adv"]) * tour_logp.sum(1)).sum().backward()
    params = AC.named_parameters(mods)
    assert len(params) == AC.N_KEYS[D]
    for key, p in params.items():
        assert p.grad is not None, key
        _close("grad " + key, p.grad, z["grad_" + key])


# ---- the wrapper and the C entries -----------------------------------------------------------------------------------------
def test_exports_and_signatures():
    L = _lib.lib()
    for name in ("tap_pointer_scores_static", "tap_pointer_scores_static_backward", "tap_pointer_scores_static_backward_scratch"):
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(L, name)
    assert list(inspect.signature(T.pointer_scores_static).parameters) == ["xs", "bits", "G", "g", "M", "k", "q", "va", "vp", "rows"]
    assert T.rollout.pointer_scores_static is T.pointer_scores_static and "pointer_scores_static" in T.__all__
    assert T.StaticFold is tools.StaticFold and "StaticFold" in T.__all__
    assert list(inspect.signature(T.Pointer.fold_static).parameters) == ["self", "static_encoder", "static_input"]
    ok = T.rollout.pointer_scores_static_supported
    assert ok(30, 20, 128, 2) and ok(128, 256, 64, 8) and ok(10, 4, 256, 1)
    assert not ok(30, 20, 128, 0) and not ok(30, 20, 128, 9) and not ok(30, 20, 96, 2) and not ok(30, 22, 128, 2)


def test_wrapper_argument_errors_before_any_launch():
    B, nR, Hd, rows, S = 3, 20, 64, 30, 2
    xs, bits = torch.ones(B, S, nR), torch.zeros(B, nR, dtype=torch.int64)
    G, g = torch.zeros(3 * Hd, S), torch.zeros(3 * Hd)
    Mf, k, q, v = torch.zeros(3 * Hd, rows), torch.zeros(3 * Hd), torch.zeros(B, Hd), torch.zeros(Hd)
    f = T.pointer_scores_static
    with pytest.raises(TypeError):
        f(xs, bits.to(torch.int32), G, g, Mf, k, q, v, v)                             # the dtype of bits
    for bad in (torch.zeros(3 * Hd, S + 1), torch.zeros(Hd, S), torch.zeros(S, 3 * Hd), torch.zeros(3 * Hd, S, dtype=torch.int64)):
        with pytest.raises(ValueError):
            f(xs, bits, bad, g, Mf, k, q, v, v)                                       # the shape of G
    for bad in (torch.zeros(Hd), torch.zeros(3 * Hd, 1), torch.zeros(3 * Hd + 1)):
        with pytest.raises(ValueError):
            f(xs, bits, G, bad, Mf, k, q, v, v)                                       # the shape of g
    for s in (0, 9):
        with pytest.raises(ValueError):
            f(torch.ones(B, s, nR), bits, torch.zeros(3 * Hd, s), g, Mf, k, q, v, v)  # S outside 1 .. 8
    for bad in (torch.ones(B, nR), torch.ones(B, S, nR, 1), torch.ones(B + 1, S, nR), torch.ones(B, S, nR + 4),
                torch.ones(B, S, nR, dtype=torch.int64)):
        with pytest.raises(ValueError):
            f(bad, bits, G, g, Mf, k, q, v, v)                                        # xs not a floating (B, S, nR)
    with pytest.raises(ValueError):
        f(xs, bits, G, g, Mf, k, q, v, v, rows=29)
    with pytest.raises(ValueError):
        f(xs, bits, G, g, torch.zeros(3 * Hd, 70), k, q, v, v)                        # two planes wanted, one given
    with pytest.raises(ValueError):
        f(xs, bits, torch.zeros(96, S), torch.zeros(96), torch.zeros(96, rows), torch.zeros(96), torch.zeros(B, 32), torch.zeros(32),
          torch.zeros(32))                                                            # Hd 32: no kernel
    # well-formed arguments on the host: refused loudly, there is no CPU path
    with pytest.raises(T.TapError):
        f(xs, bits, G, g, Mf, k, q, v, v)


def test_host_side_checks_need_no_device():
    """the C entries' checks in the header's order, with a null context and host addresses that are never dereferenced"""
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED

    def fwd(B, nR, rows, Hd, S, bufs=None):
        b = [None] * 12 if bufs is None else bufs
        return L.tap_pointer_scores_static(None, b[0], b[1], B, nR, rows, Hd, S, *b[2:12], None)

    def bwd(B, nR, rows, Hd, S, bufs=None, scr=None, nbytes=0):
        b = [None] * 16 if bufs is None else bufs
        return L.tap_pointer_scores_static_backward(None, b[0], b[1], B, nR, rows, Hd, S, *b[2:16], scr, nbytes, None)
    for f in (fwd, bwd):
        # 1. the dimensions, S < 1 among them, before anything else
        assert f(-1, 20, 30, 128, 2) == inv
        for dims in ((0, 30, 128, 2), (20, 0, 128, 2), (20, 30, 0, 2), (20, 30, 128, 0), (20, 30, 128, -1)):
            assert f(2, *dims) == inv and f(0, *dims) == inv
        # 2. an empty batch is fine whatever the buffers and the shape are
        assert f(0, 20, 30, 128, 2) == ok and f(0, 22, 30, 128, 2) == ok and f(0, 20, 30, 100, 2) == ok and f(0, 20, 30, 128, 9) == ok
        # 3. null buffers, before the shape is looked at
        assert f(1, 20, 30, 128, 2) == inv and f(1, 22, 30, 100, 9) == inv
    for hole in range(12):
        args = [p] * 12
        args[hole] = None
        assert fwd(1, 20, 30, 128, 2, args) == inv and fwd(1, 22, 30, 100, 9, args) == inv
    for hole in range(16):
        args = [p] * 16
        args[hole] = None
        assert bwd(1, 20, 30, 128, 2, args, p, 1 << 30) == inv and bwd(1, 22, 30, 100, 9, args, p, 1 << 30) == inv
    # 4. shapes without a shadow, hidden sizes without an instantiation, S > 8
    for dims in ((20, 129, 128, 2), (22, 30, 128, 2), (260, 30, 128, 2), (20, 30, 96, 2), (20, 30, 128, 9)):
        assert fwd(2, *dims, [p] * 12) == uns
        assert bwd(2, *dims, [p] * 16, p, 1 << 30) == uns
        assert L.tap_pointer_scores_static_backward_scratch(2, *dims) == 0
    # 5. the backward's scratch, then the alignment
    need = L.tap_pointer_scores_static_backward_scratch(3, 20, 30, 128, 2)
    assert need > 0 and need % 4 == 0 and need == L.tap_pointer_scores_backward_scratch(3, 20, 30, 128)
    assert L.tap_pointer_scores_static_backward_scratch(0, 20, 30, 128, 2) == 0
    assert bwd(3, 20, 30, 128, 2, [p] * 16, p, need - 1) == inv and bwd(3, 20, 30, 128, 2, [p] * 16, None, need) == inv
    q4, q2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    for hole in range(12):
        args = [p] * 12
        args[hole] = q4 if hole == 1 else q2
        assert fwd(1, 20, 30, 128, 2, args) == inv
    args = [p] * 16
    args[12] = C.c_void_p(p.value + 8)                                # dU leaves as float4s
    assert bwd(3, 20, 30, 128, 2, args, p, need) == inv
    assert bwd(3, 20, 30, 128, 2, [p] * 16, q2, need) == inv
