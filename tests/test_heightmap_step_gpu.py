"""The 3D decoder step on the MI355X (heightmap.hip: k_decoder_step_hm) against the float64 model of
tests/heightmap_model.py.

The tolerance is the project's rule, pointer_model.tolerance, not a constant.  Per case the reference's own form (an
nn.Conv1d static encoder, the HeightmapEncoder's three convolutions, their concatenation, nn.GRU for one step, the decoder's
columns of the attention's W) is evaluated in float32 torch on the CPU; its largest error against float64 is ``e_ref``, and
the kernel must stay within 4 e_ref + 16 * 2^-24 * max |want|.  The kernel's inputs are the float64 fold of the case rounded
to float32 and ``want`` is the float64 model ON those rounded inputs.  The reference's form does not name the gates; their
e_ref is the float32 run of the model's torch form.  Each test prints its worst err / e_ref."""
import copy
import os

import numpy as np
import pytest
import torch
from torch import nn

import episode_actor_model as A
import heightmap_model as HM
import pointer_model as PM
import tap_net_amd as T
from tap_net_amd import _lib, rollout, synth, tools

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TE = 16                                 # envs per workgroup (tap_decoder.h: DEC_TE)
CANARY = 12345.0
KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (C, W, L, m, Hd, Ks, B): less than one tile; the shipped shape with a ragged second tile; heightmap_only (m = Hd, no static
# half); mul-with's four planes; Np = 9; nw = 1 and nl = 3; W != L with equal nw, nl
CASES = [(2, 5, 5, 32, 64, 3, 5), (2, 5, 5, 128, 256, 3, 19), (1, 5, 5, 64, 64, 0, 17), (4, 5, 5, 64, 128, 4, 3), (2, 10, 10, 64, 128, 3, 6),
         (1, 4, 12, 32, 64, 3, 2), (2, 5, 6, 32, 64, 3, 2)]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)


def _hits(kind, extra=0):
    return {k: v for k, v in _lib.variant_hits(DEV).items() if k[0] == kind and k[5] == extra}


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))


def _np(W, L):
    return ((W + 3) // 4) * ((L + 3) // 4)


_made = {}


def _inputs(C, W, L, m, Hd, Ks, B):
    """-> X (the reference form's inputs) and the kernel's float32 inputs (xs, hm, h, enc_w, P, c, w_hh, b_hh, wq), made once
    per case and left unchanged"""
    key = (C, W, L, m, Hd, Ks, B)
    if key not in _made:
        X = HM.make_case(B, Ks, C, W, L, m, Hd, 1000 * C + 100 * W + 10 * L + m + Hd + B)
        P, c = (np.asarray(a, np.float32) for a in HM.fold(X, np.float64))
        _made[key] = (X, (X["xs"], X["hm"], X["h"], X["enc"], P, c, X["W_hh"], X["b_hh"], X["Wq"]))
    return _made[key]


def _raw(inp, with_h=True, want_gates=True, want_enc=True):
    """the forward entry on device copies -> h', q, gates, enc (None when not asked for) as numpy; every output buffer has a
    tile of canary rows behind the batch, which must come back untouched"""
    xs, hm, h, enc_w, P, c, w_hh, b_hh, wq = inp
    B, Hd, m = hm.shape[0], wq.shape[0], enc_w[4].shape[0]
    full = [torch.full((B + TE,) + s, CANARY, device=DEV) for s in ((Hd,), (Hd,), (4, Hd), (m,))]
    outs = [f[:B] for f in full]
    C, W, L = hm.shape[1:]
    ew = [_dev(a.reshape(a.shape[0], -1) if a.ndim == 4 else a) for a in enc_w]
    rollout._decoder_hm_into(_dev(xs) if xs.shape[1] else None, _dev(hm), _dev(h) if with_h else None, ew, _dev(P), _dev(c), _dev(w_hh),
                             _dev(b_hh), _dev(wq), outs[0], outs[1], outs[2] if want_gates else None, outs[3] if want_enc else None)
    torch.cuda.synchronize()
    for f, asked in zip(full, (True, True, want_gates, want_enc)):
        assert bool((f[B:] == CANARY).all())                          # nothing past the batch
        assert asked or bool((f == CANARY).all())                     # an output that was not given is not written
    return [o.cpu().numpy() if asked else None for o, asked in zip(outs, (True, True, want_gates, want_enc))]


@pytest.mark.parametrize("C,W,L,m,Hd,Ks,B", CASES)
def test_forward(C, W, L, m, Hd, Ks, B):
    X, inp = _inputs(C, W, L, m, Hd, Ks, B)
    _, z1, z2 = HM.encode(inp[1], inp[3])
    assert (z1 > 0).any() and (z1 < 0).any() and (z2 > 0).any() and (z2 < 0).any()       # both branches of both leaky-ReLUs
    assert np.array_equal(inp[1], np.round(inp[1])) and np.abs(inp[1]).max() <= 50 and inp[1].min() < 0 < inp[1].max()
    key = (_lib.TAP_HIT_HEIGHTMAP, C, _np(W, L), Hd // 64)
    worst = 0.0
    for with_h in (True, False):
        mine = inp[:2] + (inp[2] if with_h else None,) + inp[3:]
        want = HM.step(*mine)
        with torch.no_grad():
            r32, r64 = (HM.reference_form_torch(X, d, with_h) for d in (torch.float32, torch.float64))
            g32, g64 = (HM.step_torch(_t(mine[0], d), _t(mine[1], d), _t(mine[2], d), [_t(a, d) for a in mine[3]],
                                      *(_t(a, d) for a in mine[4:]))[2] for d in (torch.float32, torch.float64))
        e = [float((a.double() - b).abs().max()) for a, b in zip(r32, r64)]
        e_ref = [e[0], e[1], float((g32.double() - g64).abs().max()), e[2]]
        _lib.variant_hits_reset(DEV)
        got = _raw(inp, with_h)
        assert _hits(_lib.TAP_HIT_HEIGHTMAP) == {key + (int(with_h), 0, 0): 1}, _lib.variant_hits(DEV)
        assert not _hits(_lib.TAP_HIT_DECODER) and not _hits(_lib.TAP_HIT_HEIGHTMAP, 1)
        for name, g, w, er in zip(("h_new", "q", "gates", "enc"), got, want, e_ref):
            assert g.dtype == np.float32 and g.shape == w.shape and np.isfinite(g).all(), name
            err = float(np.abs(g.astype(np.float64) - w).max())
            print("heightmap forward %s h %d %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
                  % ((C, W, L, m, Hd, Ks, B), with_h, name, err, er, _ratio(err, er), np.abs(w).max()))
            assert np.abs(w).max() > 0 and err <= PM.tolerance(er, w), (name, with_h, err, er)
            worst = max(worst, _ratio(err, er))
        # two calls give the same bytes; without the optional outputs h' and q are the same bytes
        again, bare = _raw(inp, with_h), _raw(inp, with_h, want_gates=False, want_enc=False)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes()
        assert bare[2] is None and bare[3] is None and got[0].tobytes() == bare[0].tobytes() and got[1].tobytes() == bare[1].tobytes()
        # after the encoder the step is tap_decoder_step's contract word for word: the same bytes from enc_out as xd
        hn, q = (torch.empty(B, Hd, device=DEV) for _ in range(2))
        gates = torch.empty(B, 4, Hd, device=DEV)
        rollout._decoder_into(_dev(inp[0]) if Ks else None, _dev(got[3]), _dev(inp[2]) if with_h else None, *(_dev(a) for a in inp[4:]),
                              hn, q, gates)
        for a, b in zip(got[:3], (hn, q, gates)):
            assert a.tobytes() == b.cpu().numpy().tobytes()
        if not with_h:
            assert np.array_equal(got[2][:, 3], np.broadcast_to(inp[7][2 * Hd:], (B, Hd)))    # the zero state: gh is exactly b_hh
        if B == 19:
            # an env's bytes do not depend on the batch around it: env 7 alone
            alone = _raw(tuple(a[7:8] for a in inp[:3]) + inp[3:], with_h)
            for a, b in zip(got, alone):
                assert a[7:8].tobytes() == b.tobytes()
    print("heightmap forward %s: worst err / e_ref %.2f" % ((C, W, L, m, Hd, Ks, B), worst))


def test_cases_cover_the_indexing():
    assert {c[4] for c in CASES} == {64, 128, 256} and {c[0] for c in CASES} == {1, 2, 4}
    assert {_np(c[1], c[2]) for c in CASES} >= {3, 4, 9} and any(c[3] == c[4] and c[5] == 0 for c in CASES)
    assert any(c[6] < TE for c in CASES) and any(c[6] > TE and c[6] % TE for c in CASES)


def test_enc_on_the_recorded_episode_equals_the_reference_module():
    """the shipped 3D actor's dynamic_decoder on the 640 height maps of tests/golden/episode_3d.npz: enc_out against the
    reference module's float64 outputs, e_ref from the same convolutions in float32 torch"""
    G = np.load(os.path.join(GOLDEN_DIR, "heightmap_encoder.npz"))
    feats = np.load(os.path.join(GOLDEN_DIR, "episode_3d.npz"))["features"]
    hm = feats.reshape(640, 2, 5, 5).astype(np.float32)
    enc_w = [G["pre_" + k] for k in KEYS]
    X, inp = _inputs(2, 5, 5, 128, 256, 3, 19)
    rng = np.random.RandomState(9)
    mine = (rng.randint(0, 6, (640, 3)).astype(np.float32), hm, np.tanh(rng.randn(640, 256)).astype(np.float32), enc_w) + inp[4:]
    want = G["pre_out"]
    with torch.no_grad():
        r32 = HM.encode_torch(_t(hm, torch.float32), [_t(a, torch.float32) for a in enc_w]).double().numpy()
    e_ref = float(np.abs(r32 - want).max())
    got = _raw(mine)
    err = float(np.abs(got[3].astype(np.float64) - want).max())
    print("heightmap recorded episode enc: err %.3g e_ref %.3g ratio %.2f max|want| %.3g" % (err, e_ref, _ratio(err, e_ref), np.abs(want).max()))
    assert got[3].shape == (640, 128) and np.abs(want).max() > 1 and err <= PM.tolerance(e_ref, want)
    full, f32 = HM.step(*mine), HM.step(*mine, dtype=np.float32)        # and the step behind it, on 40 tiles: e_ref = the float32 model's error
    for name, g, w, r in zip(("h_new", "q"), got[:2], full[:2], f32[:2]):
        assert float(np.abs(g - w).max()) <= PM.tolerance(float(np.abs(r - w).max()), w), name


def _encoder_module(enc_w, C, m, W, L, dtype, device):
    net = tools.HeightmapEncoder(C, m, (W, L))
    net.load_state_dict({k: torch.from_numpy(np.asarray(a)) for k, a in zip(KEYS, enc_w)}, strict=True)
    return net.to(device=device, dtype=dtype)


NAMES = ("xs", "hm", "h", "P", "c", "w_hh", "b_hh", "wq")


def _grads(inp, with_h, g, dtype, device):
    """autograd of L = sum(h' g[0]) + sum(q g[1]) -> {name: gradient}: on the CPU through the model's torch form (the
    reference's convolutions), on the device through rollout.decoder_step_heightmap"""
    xs, hm, h, enc_w, P, c, w_hh, b_hh, wq = inp
    C, W, L = hm.shape[1:]
    on_dev = device != "cpu"
    t = (lambda a: _dev(a)) if on_dev else (lambda a: _t(a, dtype))
    leaves = dict(zip(NAMES, (t(a) for a in (xs, hm, h, P, c, w_hh, b_hh, wq))))
    if not with_h:
        leaves["h"] = None
    if not xs.shape[1]:
        leaves["xs"] = None
    net = _encoder_module(enc_w, C, enc_w[4].shape[0], W, L, dtype, device)
    wanted = [n for n in NAMES if leaves[n] is not None]
    for n in wanted:
        leaves[n].requires_grad_(True)
    if on_dev:
        hn, q = T.decoder_step_heightmap(leaves["xs"], leaves["hm"], leaves["h"], net, *(leaves[n] for n in NAMES[3:]))
        assert hn.requires_grad and q.requires_grad
    else:
        x0 = leaves["xs"] if leaves["xs"] is not None else torch.zeros(hm.shape[0], 0, dtype=dtype)
        hn, q, _, _ = HM.step_torch(x0, leaves["hm"], leaves["h"], [dict(net.named_parameters())[k] for k in KEYS],
                                    *(leaves[n] for n in NAMES[3:]))
    ((hn * t(g[0])).sum() + (q * t(g[1])).sum()).backward()
    out = {n: (torch.zeros_like(leaves[n]) if leaves[n].grad is None else leaves[n].grad).double().cpu().numpy() for n in wanted}
    out.update({k: p.grad.double().cpu().numpy() for k, p in net.named_parameters()})
    return out


@pytest.mark.parametrize("C,W,L,m,Hd,Ks,B", CASES)
def test_backward(C, W, L, m, Hd, Ks, B):
    """dP, dc, dw_hh, db_hh, dwq, dh, dxs, dhm and the encoder's six gradients through rollout.decoder_step_heightmap against
    float64 autograd of the reference form; e_ref from its float32 CPU autograd"""
    X, inp = _inputs(C, W, L, m, Hd, Ks, B)
    g = np.random.RandomState(C + W + L + B).randn(2, B, Hd).astype(np.float32)
    worst = 0.0
    for with_h in ((True, False) if B == 19 else (True,)):
        want = _grads(inp, with_h, g, torch.float64, "cpu")
        ref32 = _grads(inp, with_h, g, torch.float32, "cpu")
        _lib.variant_hits_reset(DEV)
        got = _grads(inp, with_h, g, torch.float32, DEV)
        assert _hits(_lib.TAP_HIT_HEIGHTMAP) == {(_lib.TAP_HIT_HEIGHTMAP, C, _np(W, L), Hd // 64, int(with_h), 0, 0): 1}
        assert _hits(_lib.TAP_HIT_DECODER, 1) == {(_lib.TAP_HIT_DECODER, 0, TE, Hd // 64, int(with_h), 1, 0): 1} and not _hits(_lib.TAP_HIT_DECODER)
        assert sorted(got) == sorted(want) and len(got) == 6 + 6 + int(with_h) + int(Ks > 0)
        for name in sorted(want):
            a, w, r = got[name], want[name], ref32[name]
            assert a.shape == w.shape and np.isfinite(a).all(), name
            e, err = float(np.abs(r - w).max()), float(np.abs(a - w).max())
            print("heightmap backward %s h %d %s: err %.3g e_ref %.3g ratio %.2f max|want| %.3g"
                  % ((C, W, L, m, Hd, Ks, B), with_h, name, err, e, _ratio(err, e), np.abs(w).max()))
            if name == "w_hh" and not with_h:
                assert not a.any() and not w.any()                    # the zero state: w_hh did not enter
                continue
            assert np.abs(w).max() > 0 and err <= PM.tolerance(e, w), (name, with_h, err, e)
            worst = max(worst, _ratio(err, e))
        # hm's gradient lives on the cells the encoder reads and nowhere else
        mask = np.zeros((W, L), bool)
        mask[::4, ::4] = True
        assert not got["hm"][:, :, ~mask].any() and got["hm"][:, :, mask].any()
    print("heightmap backward %s: worst err / e_ref %.2f" % ((C, W, L, m, Hd, Ks, B), worst))


# ---- through the modules -----------------------------------------------------------------------------------------------
class Actor3D(A.Actor):
    """episode_actor_model.Actor with the reference's 3D decoder input: cat(Conv1d(3, 32, 1), HeightmapEncoder(2, 32, (5, 5)))"""

    def __init__(self, static_rows, rows, block_dim, map_shape, hidden=A.H):
        super(Actor3D, self).__init__(static_rows, rows, block_dim, int(np.prod(map_shape)), hidden)
        self.map_shape = tuple(map_shape)
        self.decoder_static_encoder = nn.Conv1d(block_dim, hidden // 2, 1)
        self.decoder_dynamic_encoder = tools.HeightmapEncoder(map_shape[0], hidden // 2, map_shape[1:])
        for mod in (self.decoder_static_encoder, self.decoder_dynamic_encoder):
            for p in mod.parameters():
                if p.dim() > 1:
                    nn.init.xavier_uniform_(p)

    def decoder_input(self, decoder_static, decoder_dynamic):
        hm = decoder_dynamic.reshape(decoder_dynamic.shape[0], *self.map_shape)
        return torch.cat((self.decoder_static_encoder(decoder_static), self.decoder_dynamic_encoder(hm)), 1)


def test_training_step_through_forward_step():
    """fold_decoder(Conv1d, HeightmapEncoder) + fold_episode + forward_step on EpisodeStepper(expand_dynamic=False), D = 3,
    B = 3, the 22-node two-plane window; teacher-forced through episode_actor_model.train_step in float64 (wanted) and float32
    (e_ref): tour_logp and the gradient of every parameter, conv1 .. conv3 included"""
    B, n, cs, seed = 3, 22, [5, 5, 200], 63
    static, dynamic = synth.rand_instances(B, n, 3, seed=seed)
    assert tuple(dynamic.shape) == (B, 66, 132)
    rng = np.random.RandomState(seed + 1)
    u, adv, ghh = rng.rand(n, B).astype(np.float32), rng.randn(B).astype(np.float32), rng.randn(1, B, A.H).astype(np.float32)
    torch.manual_seed(seed + 2)
    actor = Actor3D(int(static.shape[1]), int(dynamic.shape[1]), 3, (2, 5, 5)).train()
    assert len(list(actor.parameters())) == 8 + 6 + 6
    net = copy.deepcopy(actor).to(DEV).train()
    st, dy = static.to(DEV).contiguous(), dynamic.to(DEV).contiguous()
    env = T.BatchedContainer(B, cs, n, "C+P+S-lb-soft", "diff", device=DEV)
    state = {}

    def scorer(step, decoder_static, decoder_dynamic, **_):
        assert tuple(decoder_dynamic.shape) == (B, 2, 5, 5)
        logits, state["hh"] = net.pointer.forward_step(state["proj"], sp.dynamic_bits, state["fold"], decoder_static, decoder_dynamic,
                                                       state["hh"])
        return logits
    _lib.variant_hits_reset(DEV)
    with torch.enable_grad():
        sp = T.EpisodeStepper(st, dy, env, expand_dynamic=False)
        state["proj"] = net.pointer.project_static(net.static_encoder(st))
        P, c = net.pointer.fold_decoder(net.decoder_static_encoder, net.decoder_dynamic_encoder, combine='cat')
        state["fold"] = net.pointer.fold_episode(net.dynamic_encoder, P, c)
        state["hh"] = None
        pol = T.PointerHeadPolicy(scorer, u=_dev(u))
        out = T.run_episode(st, dy, pol, cs[0], cs[-1], stepper=sp, check=False)
        tour_logp = pol.tour_logp()
        assert tuple(tour_logp.shape) == (B, n) and tour_logp.requires_grad
        ((_dev(adv) * tour_logp.sum(1)).sum() + (state["hh"] * _dev(ghh)).sum()).backward()
    sp.check()
    count = lambda kind, extra: sum(_hits(kind, extra).values())                          # noqa: E731
    assert count(_lib.TAP_HIT_HEIGHTMAP, 0) == n and count(_lib.TAP_HIT_DECODER, 0) == 0      # n forward launches of the new kernel only
    assert count(_lib.TAP_HIT_DECODER, 1) == n and count(_lib.TAP_HIT_POINTER, 0) == n and count(_lib.TAP_HIT_POINTER, 1) == n
    tour, logp, grads = out["tour_idx"].cpu().numpy(), tour_logp.detach().double().cpu().numpy(), A.named_grads(net)
    envt = A.episode_tensors(static.numpy(), dynamic.numpy(), tour, cs)
    logp64, want = A.train_step(actor, torch.float64, static.numpy(), envt, tour, adv, ghh)
    logp32, ref32 = A.train_step(actor, torch.float32, static.numpy(), envt, tour, adv, ghh)
    assert sorted(grads) == sorted(want) and len(want) == 20 and "decoder_dynamic_encoder.conv3.weight" in want
    failed, worst = [], 0.0
    for name, got, w, r in [("tour_logp", logp, logp64, logp32)] + [(k, grads[k], want[k], ref32[k]) for k in sorted(want)]:
        assert got.shape == w.shape and np.isfinite(got).all() and np.isfinite(w).all(), name
        e, err = float(np.abs(r - w).max()), float(np.abs(got - w).max())
        tol = PM.tolerance(e, w)
        print("heightmap step path %s: err %.3g e_ref %.3g ratio %.2f tolerance %.3g max|want| %.3g" % (name, err, e, _ratio(err, e), tol,
                                                                                                      np.abs(w).max()))
        if not (np.abs(w).max() > 0 and err <= tol):
            failed.append((name, err, tol))
        worst = max(worst, _ratio(err, e))
    print("heightmap step path: worst err / e_ref %.2f" % worst)
    assert not failed, failed


def test_step_and_head_replay_from_a_hip_graph():
    B, rows, nR, H = 64, 30, 20, 128
    torch.manual_seed(71)
    net = tools.Pointer(H, H, 'shape_heightmap', 'bot').eval()
    for p in net.parameters():
        nn.init.xavier_uniform_(p) if p.dim() > 1 else nn.init.normal_(p, std=0.1)
    net = net.to(DEV)
    enc = T.DynamicBitsEncoder(rows, H).to(DEV)
    dec_s, dec_d = nn.Conv1d(3, H // 2, 1).to(DEV), tools.HeightmapEncoder(2, H // 2, (5, 5)).to(DEV)
    rng = np.random.RandomState(72)
    bits = _dev(PM.pack_bits(rng.rand(B, rows, nR) < 0.1))
    mask = _dev((rng.rand(B, nR) < 0.5).astype(np.float32))
    mask[:, 0] = 1
    us = [_dev(rng.rand(B).astype(np.float32)) for _ in range(3)]
    u = us[0].clone()
    sh, hh = torch.randn(B, H, nR, device=DEV), torch.tanh(torch.randn(1, B, H, device=DEV))
    ds, dd = torch.randint(1, 6, (B, 3, 1), device=DEV).float(), torch.randint(-50, 51, (B, 2, 5, 5), device=DEV).float()

    def step():
        logits, last = net.forward_step(proj, bits, fold, ds, dd, hh)
        ptr, logp = T.pointer_pick(logits, mask, u)
        return logits, last, ptr, logp
    with torch.no_grad():
        proj = net.project_static(sh)
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
        _lib.variant_hits_reset(DEV)
        first = step()
        assert sum(_hits(_lib.TAP_HIT_HEIGHTMAP).values()) == 1 and not _hits(_lib.TAP_HIT_DECODER)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = step()
        picks = []
        for fresh in us[1:]:
            u.copy_(fresh)                                            # refreshed uniforms, the same buffer
            for v in rec:
                v.zero_()
            graph.replay()
            torch.cuda.synchronize()
            eager = step()
            for a, b in zip(rec, eager):
                assert torch.equal(a, b)
            picks.append(rec[2].clone())
    assert torch.equal(first[0], eager[0]) and not torch.equal(picks[0], picks[1])        # the same logits, other picks
    assert bool(torch.isfinite(first[0]).all()) and float(first[0].abs().max()) > 0 and bool(torch.isfinite(eager[3]).all())
