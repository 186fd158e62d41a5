"""Dropout inside the decoder step's launch on the MI355X (decoder.hip: k_decoder_step<DecArgsDrop>, k_decoder_step_bw_drop;
heightmap.hip: k_decoder_step_hm<HmArgsDrop>) against the float64 model of tests/step_dropout_model.py.

The masks are compared bit for bit with the numpy model.  The values follow the tolerance rule of the decoder tests,
pointer_model.tolerance, not a constant: ``e_ref`` is the float32 run of the reference's form (nn.Conv1d encoders, nn.GRU,
the attention's columns) with the same explicit masks where it has its two nn.Dropout, and the kernel must stay within
4 e_ref + 16 * 2^-24 * max |want| of the float64 model on the rounded inputs.  Each test prints its err / e_ref."""
import copy

import numpy as np
import pytest
import torch

import decoder_step_model as M
import episode_actor_model as A
import heightmap_model as HM
import pointer_model as PM
import step_dropout_model as SD
import tap_net_amd as T
from tap_net_amd import _lib, rollout, tools
from test_decoder_step_gpu import _inputs, _setup
from test_episode_autograd_gpu import _loss_backward, _to
from test_heightmap_step_gpu import _inputs as _hm_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TE = 16
SEED, EPISODE, STEP = 0x1234567855AA33CC, 2 ** 32 + 5, 2          # a seed with a high half; the launch takes the episode mod 2^32
PS = [(0.1, 0.3), (0.5, 0.5)]                                    # unequal: swapped masks would show
CASES = [(2, 4, 64, 1), (2, 4, 128, 67), (3, 0, 256, 2), (2, 4, 64, 2051)]
BW_CASES = [(2, 4, 128, 67), (3, 0, 256, 2), (2, 4, 64, 2051)]
HM_CASES = [(2, 5, 5, 32, 64, 3, 3), (2, 5, 5, 128, 256, 3, 18)]  # (C, W, L, m, Hd, Ks, B)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))


def _keys(kind, extra):
    return {k for k in _lib.variant_keys(DEV) if k[0] == kind and k[5] == extra}


def _record(p, step=STEP, env_offset=0, episode=EPISODE):
    return rollout.StepDropoutRecord(torch.tensor([SEED, episode], dtype=torch.int64, device=DEV), step, p[0], p[1], env_offset)


def _raw(inp, with_h, p, step=STEP, env_offset=0):
    """tap_decoder_step_dropout on device copies -> h_out, q, gates, rnn_out, keep as numpy"""
    xs, xd, h, P, c, w_hh, b_hh, wq = inp
    B, Hd = xs.shape[0], wq.shape[0]
    hn, q, rnn = (torch.full((B, Hd), float('nan'), device=DEV) for _ in range(3))
    gates = torch.full((B, 4, Hd), float('nan'), device=DEV)
    keep = torch.full((B, 2, Hd // 64), 0x5555, dtype=torch.int64, device=DEV)
    rollout._decoder_dropout_into(_dev(xs) if xs.shape[1] else None, _dev(xd) if xd.shape[1] else None, _dev(h) if with_h else None,
                                  _dev(P), _dev(c), _dev(w_hh), _dev(b_hh), _dev(wq), _record(p, step, env_offset), hn, q, gates, rnn, keep)
    return [v.cpu().numpy() for v in (hn, q, gates, rnn, keep)]


def _check_masks(got_h, got_rnn, got_keep, keep):
    """the keep words bit for bit, and a dropped element is +0.0 by its bytes (all 32 bits zero: -0.0 would show)"""
    assert got_keep.dtype == np.int64 and np.array_equal(got_keep, SD.pack(keep))
    assert not got_h.view(np.uint32)[~keep[:, 1]].any() and not got_rnn.view(np.uint32)[~keep[:, 0]].any()
    # both checks above bite: the model's masks are fixed by (SEED, EPISODE, STEP), and every case's masks drop and keep
    # something in both planes -- at the smallest, (2, 4, 64, 1), 7 / 20 of 64 at p = (0.1, 0.3) and 35 / 34 at (0.5, 0.5)
    assert keep[:, 0].any() and keep[:, 1].any() and (~keep[:, 0]).any() and (~keep[:, 1]).any()


def _check_values(what, names, got, want, e_ref):
    worst = 0.0
    for name, g, w, e in zip(names, got, want, e_ref):
        assert g.dtype == np.float32 and g.shape == w.shape and np.isfinite(g).all(), name
        err = float(np.abs(g.astype(np.float64) - w).max())
        print("%s %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g" % (what, name, err, e, _ratio(err, e), np.abs(w).max()))
        assert np.abs(w).max() > 0 and err <= PM.tolerance(e, w), (what, name, err, e)
        worst = max(worst, _ratio(err, e))
    return worst


@pytest.mark.parametrize("Ks,Kd,Hd,B", CASES)
def test_forward(Ks, Kd, Hd, B):
    X, inp = _inputs(Ks, Kd, Hd, B)
    worst = 0.0
    for p in PS:
        keep = SD.keep_bool(SEED, EPISODE, STEP, B, Hd, *p)
        for with_h in (True, False):
            mine = inp[:2] + (inp[2] if with_h else None,) + inp[3:]
            want = SD.step(*mine, keep, *p)                                   # h_out, q, gates, rnn_out
            with torch.no_grad():
                r32, r64 = (SD.reference_form_torch(X, d, with_h, keep, *p) for d in (torch.float32, torch.float64))
                g32, g64 = (M.step_torch(*(_t(a, d) for a in mine))[2] for d in (torch.float32, torch.float64))
            e = [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)]
            e_ref = [e[0], e[1], float((g32.double() - g64).abs().max()), e[2]]
            _lib.variant_hits_reset(DEV)
            got = _raw(inp, with_h, p)
            assert _keys(_lib.TAP_HIT_DECODER, 2) == {(_lib.TAP_HIT_DECODER, 0, TE, Hd // 64, int(with_h), 2, 0)}
            assert not _keys(_lib.TAP_HIT_DECODER, 0) and len(_lib.variant_keys(DEV)) == 1
            _check_masks(got[0], got[3], got[4], keep)
            worst = max(worst, _check_values("dropout forward %s p %s h %d" % ((Ks, Kd, Hd, B), p, with_h),
                                             ("h_out", "q", "gates", "rnn_out"), got[:4], want, e_ref))
            again = _raw(inp, with_h, p)
            for a, b in zip(got, again):
                assert a.tobytes() == b.tobytes()                             # two calls give the same bytes
            if B > 1:
                # an env's bytes depend on its index in the whole batch, not on the call: the last env alone
                alone = _raw(tuple(a[-1:] for a in inp[:3]) + inp[3:], with_h, p, env_offset=B - 1)
                for a, b in zip(got, alone):
                    assert a[-1:].tobytes() == b.tobytes()
            nxt = _raw(inp, with_h, p, step=STEP + 1)
            assert np.array_equal(nxt[4], SD.keep_words(SEED, EPISODE, STEP + 1, B, Hd, *p)) and not np.array_equal(nxt[4], got[4])
    print("dropout forward %s: worst err / e_ref %.2f" % ((Ks, Kd, Hd, B), worst))


def test_p_zero_is_the_plain_launch_byte_for_byte():
    Ks, Kd, Hd, B = 2, 4, 128, 67
    _, inp = _inputs(Ks, Kd, Hd, B)
    for with_h in (True, False):
        hn, q = (torch.empty(B, Hd, device=DEV) for _ in range(2))
        gates = torch.empty(B, 4, Hd, device=DEV)
        rollout._decoder_into(_dev(inp[0]), _dev(inp[1]), _dev(inp[2]) if with_h else None, *(_dev(a) for a in inp[3:]), hn, q, gates)
        _lib.variant_hits_reset(DEV)
        got = _raw(inp, with_h, (0.0, 0.0))
        assert _lib.variant_keys(DEV) == {(_lib.TAP_HIT_DECODER, 0, TE, Hd // 64, int(with_h), 2, 0)}
        for a, b in zip(got[:3] + [got[3]], (hn, q, gates, hn)):
            assert a.tobytes() == b.cpu().numpy().tobytes()
        assert (got[4] == -1).all()


def _hm_raw(inp, with_h, p, step=STEP, env_offset=0):
    xs, hm, h, enc_w, P, c, w_hh, b_hh, wq = inp
    B, Hd, m = hm.shape[0], wq.shape[0], enc_w[4].shape[0]
    hn, q, rnn = (torch.full((B, Hd), float('nan'), device=DEV) for _ in range(3))
    gates = torch.full((B, 4, Hd), float('nan'), device=DEV)
    enc = torch.full((B, m), float('nan'), device=DEV)
    keep = torch.full((B, 2, Hd // 64), 0x5555, dtype=torch.int64, device=DEV)
    ew = [_dev(a.reshape(a.shape[0], -1) if a.ndim == 4 else a) for a in enc_w]
    rollout._decoder_hm_dropout_into(_dev(xs) if xs.shape[1] else None, _dev(hm), _dev(h) if with_h else None, ew, _dev(P), _dev(c),
                                     _dev(w_hh), _dev(b_hh), _dev(wq), _record(p, step, env_offset), hn, q, gates, enc, rnn, keep)
    return [v.cpu().numpy() for v in (hn, q, gates, enc, rnn, keep)]


@pytest.mark.parametrize("C,W,L,m,Hd,Ks,B", HM_CASES)
def test_heightmap_forward(C, W, L, m, Hd, Ks, B):
    X, inp = _hm_inputs(C, W, L, m, Hd, Ks, B)
    Np = ((W + 3) // 4) * ((L + 3) // 4)
    worst = 0.0
    for p in PS:
        keep = SD.keep_bool(SEED, EPISODE, STEP, B, Hd, *p)
        for with_h in (True, False):
            mine = inp[:2] + (inp[2] if with_h else None,) + inp[3:]
            hn, _, gates, enc = HM.step(*mine)
            h_out, q, rnn = SD.masked(hn, inp[8], keep, *p)
            want = (h_out, q, gates, enc, rnn)
            with torch.no_grad():
                ref = {}
                for d in (torch.float32, torch.float64):
                    h_ref, _, enc_ref = HM.reference_form_torch(X, d, with_h)
                    ref[d] = SD.masked_torch(h_ref, _t(X["Wq"], d), torch.from_numpy(keep), *p) + (enc_ref,)
                g32, g64 = (HM.step_torch(_t(mine[0], d), _t(mine[1], d), _t(mine[2], d), [_t(a, d) for a in mine[3]],
                                          *(_t(a, d) for a in mine[4:]))[2] for d in (torch.float32, torch.float64))
            e = [float((a.double() - b).abs().max()) for a, b in zip(ref[torch.float32], ref[torch.float64])]   # h_out, q, rnn, enc
            e_ref = [e[0], e[1], float((g32.double() - g64).abs().max()), e[3], e[2]]
            _lib.variant_hits_reset(DEV)
            got = _hm_raw(inp, with_h, p)
            assert _lib.variant_keys(DEV) == {(_lib.TAP_HIT_HEIGHTMAP, C, Np, Hd // 64, int(with_h), 2, 0)}
            _check_masks(got[0], got[4], got[5], keep)
            worst = max(worst, _check_values("dropout heightmap %s p %s h %d" % ((C, W, L, m, Hd, Ks, B), p, with_h),
                                             ("h_out", "q", "gates", "enc", "rnn_out"), got[:5], want, e_ref))
            for a, b in zip(got, _hm_raw(inp, with_h, p)):
                assert a.tobytes() == b.tobytes()
            alone = _hm_raw(tuple(a[-1:] for a in inp[:3]) + inp[3:], with_h, p, env_offset=B - 1)
            for a, b in zip(got, alone):
                assert a[-1:].tobytes() == b.tobytes()
            nxt = _hm_raw(inp, with_h, p, step=STEP + 1)
            assert np.array_equal(nxt[5], SD.keep_words(SEED, EPISODE, STEP + 1, B, Hd, *p)) and not np.array_equal(nxt[5], got[5])
    # p = 0: the bytes of the plain height-map launch
    hn, q = (torch.empty(B, Hd, device=DEV) for _ in range(2))
    ew = [_dev(a.reshape(a.shape[0], -1) if a.ndim == 4 else a) for a in inp[3]]
    rollout._decoder_hm_into(_dev(inp[0]), _dev(inp[1]), _dev(inp[2]), ew, *(_dev(a) for a in inp[4:]), hn, q, None, None)
    zero = _hm_raw(inp, True, (0.0, 0.0))
    assert zero[0].tobytes() == hn.cpu().numpy().tobytes() and zero[1].tobytes() == q.cpu().numpy().tobytes() and (zero[5] == -1).all()
    print("dropout heightmap %s: worst err / e_ref %.2f" % ((C, W, L, m, Hd, Ks, B), worst))


@pytest.mark.parametrize("Ks,Kd,Hd,B", BW_CASES)
def test_backward_launch(Ks, Kd, Hd, B):
    """the launch's own outputs against the closed form in float64, with g composed from the masks; the bound is the plain
    backward launch's (test_decoder_step_gpu): every output is g times factors of at most 1 (h - n: 2) and, for da_r, gh_n --
    at most 8 roundings there and 3 more in g (two products and their sum), each 2^-24 of that: 16 covers them"""
    _, inp = _inputs(Ks, Kd, Hd, B)
    p = PS[0]
    rng = np.random.RandomState(Ks + Kd + B)
    g_h, g_r = (rng.randn(B, Hd).astype(np.float32) for _ in range(2))
    keep = SD.keep_bool(SEED, EPISODE, STEP, B, Hd, *p)
    s_rnn, s_hh = SD.scale(p[0]), SD.scale(p[1])
    for with_h in (True, False):
        gates = _raw(inp, with_h, p)[2]
        outs = []
        _lib.variant_hits_reset(DEV)
        for _ in range(2):
            o = [torch.full(s, float('nan'), device=DEV) for s in ((B, 3 * Hd), (B, Hd), (B, Hd))]
            rollout._decoder_dropout_backward_into(_dev(gates), _dev(inp[2]) if with_h else None, _dev(g_h), _dev(g_r), _dev(SD.pack(keep)),
                                                   s_rnn, s_hh, *o)
            outs.append([v.cpu().numpy() for v in o])
        assert _lib.variant_keys(DEV) == {(_lib.TAP_HIT_DECODER, 0, TE, Hd // 64, int(with_h), 3, 0)}
        for a, b in zip(*outs):
            assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
        r, z, n, ghn = (gates[:, i].astype(np.float64) for i in range(4))
        h = inp[2].astype(np.float64) if with_h else 0.0
        g = keep[:, 1] * s_hh * g_h.astype(np.float64) + keep[:, 0] * s_rnn * g_r.astype(np.float64)
        dan = g * (1 - z) * (1 - n * n)
        want = [np.concatenate((dan * ghn * r * (1 - r), g * (h - n) * z * (1 - z), dan), axis=1), dan * r, g * z]
        bound = 16 * PM.U32 * float(np.abs(g).max()) * max(1.0, float(np.abs(ghn).max()))
        for a, w in zip(outs[0], want):
            assert np.abs(w).max() > 0 and float(np.abs(a - w).max()) <= bound
        both = ~keep[:, 0] & ~keep[:, 1]                                  # dropped from both: an exact zero gradient
        assert both.any() and not outs[0][2][both].any() and not outs[0][0].reshape(B, 3, Hd)[:, 2][both].any()


def _grads(fn, leaves, wanted, g, to):
    for n in wanted:
        leaves[n].requires_grad_(True)
    h_out, q = fn(leaves)[:2]
    ((h_out * to(g[0])).sum() + (q * to(g[1])).sum()).backward()
    return {n: leaves[n].grad.detach().double().cpu().numpy() for n in wanted}


def test_gradients_through_decoder_step_dropout():
    """every gradient of rollout.decoder_step_dropout -- P, c, w_hh, b_hh, wq and h -- against float64 autograd of the model
    with the same masks; e_ref from its float32 CPU autograd"""
    Ks, Kd, Hd, B = 2, 4, 128, 67
    _, inp = _inputs(Ks, Kd, Hd, B)
    p = PS[0]
    names = ("xs", "xd", "h", "P", "c", "w_hh", "b_hh", "wq")
    wanted = names[2:]
    g = np.random.RandomState(11).randn(2, B, Hd).astype(np.float32)
    keep = SD.keep_bool(SEED, EPISODE, STEP, B, Hd, *p)
    cpu = {d: _grads(lambda lv: SD.step_torch(*(lv[n] for n in names), torch.from_numpy(keep), *p),
                     dict(zip(names, (_t(a, d) for a in inp))), wanted, g, lambda a, d=d: _t(a, d)) for d in (torch.float64, torch.float32)}
    _lib.variant_hits_reset(DEV)
    got = _grads(lambda lv: T.decoder_step_dropout(*(lv[n] for n in names), _record(p)), dict(zip(names, (_dev(a) for a in inp))), wanted, g, _dev)
    assert _keys(_lib.TAP_HIT_DECODER, 2) and _keys(_lib.TAP_HIT_DECODER, 3) and not _keys(_lib.TAP_HIT_DECODER, 0) and \
        not _keys(_lib.TAP_HIT_DECODER, 1)
    for name in wanted:
        w, e = cpu[torch.float64][name], float(np.abs(cpu[torch.float32][name] - cpu[torch.float64][name]).max())
        err = float(np.abs(got[name] - w).max())
        print("dropout backward %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g" % (name, err, e, _ratio(err, e), np.abs(w).max()))
        assert np.abs(w).max() > 0 and err <= PM.tolerance(e, w), (name, err, e)


def test_gradients_through_decoder_step_heightmap_dropout():
    """the same through the height-map form: the encoder's six parameters too (its backward receives dgi as before)"""
    C, W, L, m, Hd, Ks, B = HM_CASES[0]
    X, inp = _hm_inputs(C, W, L, m, Hd, Ks, B)
    p = PS[0]
    keep = SD.keep_bool(SEED, EPISODE, STEP, B, Hd, *p)
    g = np.random.RandomState(12).randn(2, B, Hd).astype(np.float32)
    names = ("xs", "hm", "h", "w1", "b1", "w2", "b2", "w3", "b3", "P", "c", "w_hh", "b_hh", "wq")
    wanted = names[2:]
    flat = (inp[0], inp[1], inp[2]) + tuple(inp[3]) + tuple(inp[4:])

    def model(lv):
        hn, _, _, _ = HM.step_torch(lv["xs"], lv["hm"], lv["h"], [lv[n] for n in names[3:9]], *(lv[n] for n in names[9:]))
        return SD.masked_torch(hn, lv["wq"], torch.from_numpy(keep), *p)

    def device(lv):
        enc = tools.HeightmapEncoder(C, m, (W, L))
        for conv, w, b in ((enc.conv1, "w1", "b1"), (enc.conv2, "w2", "b2"), (enc.conv3, "w3", "b3")):
            conv.weight, conv.bias = lv[w], lv[b]                             # (the leaves themselves: their .grad is read)
        return T.decoder_step_heightmap_dropout(lv["xs"], lv["hm"], lv["h"], enc, *(lv[n] for n in names[9:]), _record(p))
    cpu = {d: _grads(model, dict(zip(names, (_t(a, d) for a in flat))), wanted, g, lambda a, d=d: _t(a, d)) for d in (torch.float64, torch.float32)}
    _lib.variant_hits_reset(DEV)
    leaves = {n: torch.nn.Parameter(_dev(a)) if n in names[3:9] else _dev(a) for n, a in zip(names, flat)}
    got = _grads(device, leaves, wanted, g, _dev)
    assert _keys(_lib.TAP_HIT_HEIGHTMAP, 2) and _keys(_lib.TAP_HIT_DECODER, 3) and not _keys(_lib.TAP_HIT_HEIGHTMAP, 0) and \
        not _keys(_lib.TAP_HIT_DECODER, 1)
    for name in wanted:
        w, e = cpu[torch.float64][name], float(np.abs(cpu[torch.float32][name] - cpu[torch.float64][name]).max())
        err = float(np.abs(got[name] - w).max())
        print("dropout heightmap backward %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g" % (name, err, e, _ratio(err, e), np.abs(w).max()))
        assert np.abs(w).max() > 0 and err <= PM.tolerance(e, w), (name, err, e)


# ---- through the modules -----------------------------------------------------------------------------------------------
def _step_path(S, actor, seed):
    """test_decoder_step_gpu's step path with the actor's dropouts active: forward_step_dropout + the head per step"""
    net = copy.deepcopy(actor).to(DEV).train()
    static, dynamic, u = S["static"].to(DEV).contiguous(), S["dynamic"].to(DEV).contiguous(), _to(S["u"])
    env = T.BatchedContainer(S["B"], S["cs"], S["n"], "C+P+S-lb-soft", "diff", device=DEV)
    sd = T.StepDropout(seed, DEV)
    sd.next_episode()
    state = {}

    def scorer(step, decoder_static, decoder_dynamic, **_):
        logits, state["hh"] = net.pointer.forward_step_dropout(state["proj"], sp.dynamic_bits, state["fold"], decoder_static,
                                                               decoder_dynamic, state["hh"], sd)
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
        sd.next_episode()                                                 # a pending backward holds the masks, not the state
        _loss_backward(S, tour_logp, state["hh"])
    sp.check()
    assert sd.step == 0 and sd.state.tolist() == [seed, 2]
    hits = {(kind, extra): sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == kind and k[5] == extra)
            for kind in (_lib.TAP_HIT_DECODER, _lib.TAP_HIT_HEIGHTMAP, _lib.TAP_HIT_POINTER) for extra in (0, 1, 2, 3)}
    n = S["n"]
    assert hits[(_lib.TAP_HIT_DECODER, 2)] == n and hits[(_lib.TAP_HIT_DECODER, 3)] == n, hits
    assert hits[(_lib.TAP_HIT_DECODER, 0)] == 0 and hits[(_lib.TAP_HIT_DECODER, 1)] == 0, hits
    assert hits[(_lib.TAP_HIT_POINTER, 0)] == n and hits[(_lib.TAP_HIT_POINTER, 1)] == n, hits
    assert not any(hits[(_lib.TAP_HIT_HEIGHTMAP, e)] for e in range(4)), hits
    return out["tour_idx"].cpu().numpy(), tour_logp.detach().double().cpu().numpy(), A.named_grads(net)


@pytest.mark.parametrize("D,B", [(2, 67), (3, 3)])
def test_training_step_through_forward_step_dropout(D, B):
    """test_training_step_through_forward_step's set-up with the actor's dropouts at the reference's 0.1, in train():
    teacher-forced through step_dropout_model.train_step in float64 (wanted) and float32 (e_ref) with the model's masks --
    tour_logp and the gradient of every parameter"""
    S = _setup(D, B, 41 if D == 2 else 63)
    seed = 2024
    actor = SD.with_dropout(S["actor"], 0.1, 0.1)
    tour, logp, grads = _step_path(S, actor, seed)
    st, dy = S["static"].numpy(), S["dynamic"].numpy()
    env = A.episode_tensors(st, dy, tour, S["cs"])
    logp64, want = SD.train_step(actor, torch.float64, st, env, tour, S["adv"], S["ghh"], seed, 1)
    logp32, ref32 = SD.train_step(actor, torch.float32, st, env, tour, S["adv"], S["ghh"], seed, 1)
    assert sorted(grads) == sorted(want) and len(want) == 8 + 4 * 2
    rows = [("tour_logp", logp, logp64, logp32)] + [(name, grads[name], want[name], ref32[name]) for name in sorted(want)]
    failed, worst = [], ("", 0.0)
    for name, got, w, r in rows:
        assert got.shape == w.shape and np.isfinite(got).all() and np.isfinite(w).all(), name
        e, err = float(np.abs(r - w).max()), float(np.abs(got - w).max())
        tol = PM.tolerance(e, w)
        print("dropout step path %dD %s: err %.3g e_ref %.3g ratio %.2f tolerance %.3g max|want| %.3g"
              % (D, name, err, e, _ratio(err, e), tol, np.abs(w).max()))
        if not (np.abs(w).max() > 0 and err <= tol):
            failed.append((name, err, tol))
        if _ratio(err, e) > worst[1]:
            worst = (name, _ratio(err, e))
    print("dropout step path %dD: worst err / e_ref %.2f (%s)" % (D, worst[1], worst[0]))
    assert not failed, failed
    # the masks matter: the same tour without dropout misses the GRU's gradients by far more than the tolerance
    _, plain = A.train_step(S["actor"], torch.float64, st, env, tour, S["adv"], S["ghh"])
    for name in ("pointer.gru.weight_hh_l0", "pointer.gru.weight_ih_l0"):
        tol = PM.tolerance(float(np.abs(ref32[name] - want[name]).max()), want[name])
        assert float(np.abs(plain[name] - want[name]).max()) > 100 * tol, name


def test_forward_step_dropout_with_a_heightmap_fold():
    """a 3D actor's step through the module: forward_step_dropout hands the record to the height-map launch.  Against the
    reference's ``forward`` on the CPU with the model's masks where it has its two nn.Dropout, float64 (wanted) and float32
    (e_ref): logits, last_hh and every parameter's gradient; one (30, ..., 2) and one (29, ..., 3) launch, none of 0 / 1"""
    B, rows, nR, H, p = 5, 30, 20, 128, (0.1, 0.3)
    torch.manual_seed(81)
    net = tools.Pointer(H, H, 'shape_heightmap', 'bot').train()
    net.drop_rnn.p, net.drop_hh.p = p
    enc = T.DynamicBitsEncoder(rows, H)
    dec_s, dec_d = torch.nn.Conv1d(3, H // 2, 1), tools.HeightmapEncoder(2, H // 2, (5, 5))
    mods = (net, enc, dec_s, dec_d)
    for m in mods:
        for q in m.parameters():
            torch.nn.init.xavier_uniform_(q) if q.dim() > 1 else torch.nn.init.normal_(q, std=0.1)
    rng = np.random.RandomState(82)
    dyn = rng.rand(B, rows, nR) < 0.1
    sh, hh = torch.randn(B, H, nR), torch.tanh(torch.randn(1, B, H))
    ds, dd = torch.randint(1, 6, (B, 3, 1)).float(), torch.randint(-50, 51, (B, 2, 5, 5)).float()
    gl, gh = torch.randn(B, nR), torch.randn(1, B, H)
    seed, keep = 4242, SD.keep_bool(4242, 1, 0, B, H, *p)

    def named(ms):
        return {"%d.%s" % (i, n): q.grad.detach().double().cpu().numpy() for i, m in enumerate(ms) for n, q in m.named_parameters()}

    def reference(dtype):
        n2, e2, s2, d2 = (copy.deepcopy(m).to(dtype).train() for m in mods)
        n2.drop_rnn, n2.drop_hh = SD.MaskDrop(p[0]), SD.MaskDrop(p[1])
        n2.drop_rnn.kept, n2.drop_hh.kept = torch.from_numpy(keep[:, 0]), torch.from_numpy(keep[:, 1])
        hidden = torch.cat((s2(ds.to(dtype)), d2(dd.to(dtype))), 1)
        logits, last = n2(sh.to(dtype), e2(torch.from_numpy(dyn).to(dtype)), hidden, hh.to(dtype))
        ((logits * gl.to(dtype)).sum() + (last * gh.to(dtype)).sum()).backward()
        return [logits.detach().double().numpy(), last.detach().double().numpy()], named((n2, e2, s2, d2))
    want, gwant = reference(torch.float64)
    ref32, gref32 = reference(torch.float32)
    n3, e3, s3, d3 = (copy.deepcopy(m).to(DEV).train() for m in mods)
    sd = T.StepDropout(seed, DEV)
    sd.next_episode()
    _lib.variant_hits_reset(DEV)
    proj = n3.project_static(sh.to(DEV))
    fold = n3.fold_episode(e3, *n3.fold_decoder(s3, d3))
    bits = _dev(PM.pack_bits(dyn))
    logits, last = n3.forward_step_dropout(proj, bits, fold, ds.to(DEV), dd.to(DEV), hh.to(DEV), sd)
    assert sd.step == 1
    ((logits * gl.to(DEV)).sum() + (last * gh.to(DEV)).sum()).backward()
    assert _keys(_lib.TAP_HIT_HEIGHTMAP, 2) == {(_lib.TAP_HIT_HEIGHTMAP, 2, 4, H // 64, 1, 2, 0)}, _lib.variant_keys(DEV)
    assert _keys(_lib.TAP_HIT_DECODER, 3) == {(_lib.TAP_HIT_DECODER, 0, TE, H // 64, 1, 3, 0)}
    assert not any(_keys(kind, extra) for kind in (_lib.TAP_HIT_DECODER, _lib.TAP_HIT_HEIGHTMAP) for extra in (0, 1))
    assert not _keys(_lib.TAP_HIT_DECODER, 2) and not _keys(_lib.TAP_HIT_HEIGHTMAP, 3)
    got_last = last.detach().cpu().numpy()
    assert not got_last[0].view(np.uint32)[~keep[:, 1]].any() and (~keep[:, 1]).any()
    rows_ = [("logits", logits.detach().double().cpu().numpy(), want[0], ref32[0]), ("last_hh", got_last.astype(np.float64), want[1], ref32[1])]
    ggot = named((n3, e3, s3, d3))
    assert sorted(ggot) == sorted(gwant) and len(gwant) == 8 + 2 + 2 + 6
    rows_ += [(k, ggot[k], gwant[k], gref32[k]) for k in sorted(gwant)]
    failed, worst = [], 0.0
    for name, g, w, r in rows_:
        e, err = float(np.abs(r - w).max()), float(np.abs(g - w).max())
        print("dropout heightmap module %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g" % (name, err, e, _ratio(err, e), np.abs(w).max()))
        if not (g.shape == w.shape and np.abs(w).max() > 0 and err <= PM.tolerance(e, w)):
            failed.append((name, err, e))
        worst = max(worst, _ratio(err, e))
    print("dropout heightmap module: worst err / e_ref %.2f" % worst)
    assert not failed, failed


def test_a_state_on_another_device_is_refused_before_any_launch():
    """a StepDropout on the host with the step's tensors on the device: ValueError from the module and from the function
    forms, and no launch is recorded"""
    Ks, Kd, Hd, B = 2, 4, 64, 1
    _, inp = _inputs(Ks, Kd, Hd, B)
    host = T.StepDropout(3, "cpu")
    _lib.variant_hits_reset(DEV)
    with pytest.raises(ValueError, match="lives on cpu"):
        T.decoder_step_dropout(*(_dev(a) for a in inp), host.take_step(0.1, 0.1))
    outs = [torch.zeros(B, Hd, device=DEV) for _ in range(2)]
    with pytest.raises(ValueError, match="lives on cpu"):
        rollout._decoder_dropout_into(*(_dev(a) for a in inp), rollout.StepDropoutRecord(host.state, 0, 0.1, 0.1, 0), *outs, None, None,
                                      torch.zeros(B, 2, 1, dtype=torch.int64, device=DEV))
    net = tools.Pointer(64, 64, 'shape_heightmap', 'bot').to(DEV).train()
    enc = T.DynamicBitsEncoder(30, 64).to(DEV)
    dec_s, dec_d = torch.nn.Conv1d(2, 32, 1).to(DEV), torch.nn.Conv1d(4, 32, 1).to(DEV)
    with torch.no_grad():
        proj = net.project_static(torch.randn(B, 64, 20, device=DEV))
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
        bits = _dev(PM.pack_bits(np.zeros((B, 30, 20), bool)))
        with pytest.raises(ValueError, match="state lives on cpu"):
            net.forward_step_dropout(proj, bits, fold, torch.ones(B, 2, 1, device=DEV), torch.ones(B, 4, 1, device=DEV), None, host)
    assert not _keys(_lib.TAP_HIT_DECODER, 2) and not _keys(_lib.TAP_HIT_DECODER, 0)


def test_episode_head_and_two_steps_replay_from_a_hip_graph():
    B, rows, nR, H = 64, 30, 20, 128
    p = 0.1
    torch.manual_seed(61)
    net = tools.Pointer(H, H, 'shape_heightmap', 'bot', dropout=p).train()
    for q in net.parameters():
        torch.nn.init.xavier_uniform_(q) if q.dim() > 1 else torch.nn.init.normal_(q, std=0.1)
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
    seed = 777

    def episode(sd):
        sd.next_episode()
        out, last = [], hh
        for t in range(2):
            words = rollout.dropout_keep_words(sd.state, t, B, H, p, p)       # the torch form, captured beside the launches
            logits, last = net.forward_step_dropout(proj, bits, fold, ds, dd, last, sd)
            ptr, logp = T.pointer_pick(logits, mask, u)
            out += [words, logits, last, ptr, logp]
        return out
    with torch.no_grad():
        proj = net.project_static(sh)
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
        sd = T.StepDropout(seed, DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            episode(sd)
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = episode(sd)
        torch.cuda.synchronize()
        e0 = int(sd.state[1])
        replays = []
        for i in (1, 2):
            for v in rec:
                v.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert sd.state.tolist() == [seed, e0 + i]
            replays.append([v.clone() for v in rec])
            for t in range(2):
                keep = SD.keep_bool(seed, e0 + i, t, B, H, p, p)
                assert np.array_equal(rec[5 * t].cpu().numpy(), SD.pack(keep))
                last = rec[5 * t + 2][0].cpu().numpy()
                # drop_hh's mask, read off last_hh (a kept element may be an honest zero: z saturated on a dropped h)
                assert not last.view(np.uint32)[~keep[:, 1]].any() and np.count_nonzero(last[keep[:, 1]]) > 0.9 * keep[:, 1].sum()
        assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[0][1], replays[1][1])
        fresh = T.StepDropout(seed, DEV)
        fresh.state[1] = e0
        eager = episode(fresh)
        for a, b in zip(replays[0], eager):
            assert torch.equal(a, b)
    assert bool(torch.isfinite(eager[1]).all()) and float(eager[1].abs().max()) > 0 and bool(torch.isfinite(eager[4]).all())
