"""The state critic without a GPU: the module against the reference's recorded critic (tests/golden/critic_*.npz), its
state dict, fold() against the numpy / torch models of tests/critic_model.py, the exports, and the C entries' host-side
checks."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import critic_model as M
import golden_util
import tap_net_amd as T
from tap_net_amd import _lib, tools

KEYS = ["static_encoder.conv.weight", "static_encoder.conv.bias", "dynamic_encoder.conv.weight", "dynamic_encoder.conv.bias",
        "decoder.conv.weight", "decoder.conv.bias", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0",
        "attention.v", "attention.W", "fc.0.weight", "fc.0.bias", "fc.2.weight", "fc.2.bias"]
FIXTURES = ["critic_%dd_%s.npz" % (D, ws) for D in (2, 3) for ws in ("xavier", "sharp")]


def _fixture(name):
    z = golden_util.load(name)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")}
    D = int(z["static_input"].shape[1])
    net = tools.StateCritic(D, int(z["dynamic"].shape[1]), int(sd["attention.v"].shape[2]), n_process_blocks=int(z["p"].shape[1]))
    return z, D, sd, net


def _xavier_(module, seed):
    torch.manual_seed(seed)
    for p in module.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    return module


@pytest.mark.parametrize("name", FIXTURES)
def test_strict_load_of_the_recorded_state_dict(name):
    z, D, sd, net = _fixture(name)
    assert sorted(sd) == sorted(KEYS) and sorted(net.state_dict()) == sorted(KEYS)
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(v.dtype is torch.float32 for v in sd.values())
    assert tuple(z["static_input"].shape) == ((19, 2, 20) if D == 2 else (17, 3, 60)) and int(z["p"].shape[1]) == 3
    assert float(z["s_spread"].min()) > (1.0 if "sharp" in name else 0.05)       # neither set has a flat softmax
    assert z["pretrained_s_spread"].tolist() == [0.0, 0.0]                      # (make_golden_critic.py: the checkpoints' v and W are zeros)


def test_module_at_the_pretrained_sizes_has_the_recorded_keys_and_shapes():
    z = golden_util.load(FIXTURES[0])
    by_dir = {}
    for line in z["pretrained_keys"]:
        d, k, shape = str(line).split("|")
        by_dir.setdefault(d, {})[k] = tuple(int(v) for v in shape.split("x"))
    assert len(by_dir) == 2
    every = dict(by_dir)
    for line in golden_util.load(FIXTURES[2])["pretrained_keys"]:
        d, k, shape = str(line).split("|")
        every.setdefault(d, {})[k] = tuple(int(v) for v in shape.split("x"))
    assert len(every) == 4
    for d, rec in every.items():
        net = T.realCritic(rec["static_encoder.conv.weight"][1], rec["dynamic_encoder.conv.weight"][1], rec["attention.v"][2])
        mine = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        assert mine == rec and list(net.state_dict()) == list(rec), d
        assert int(d[0]) == rec["static_encoder.conv.weight"][1]


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_path_reproduces_the_reference_in_float64(name):
    """every sum has at most 192 terms of O(1): far below 1e-12 relative"""
    z, D, sd, net = _fixture(name)
    net.load_state_dict(sd, strict=True)
    net = net.double().eval()
    x, dyn, a = (torch.from_numpy(z[k]) for k in ("static_input", "dynamic", "a"))
    ps = []
    real = torch.softmax
    try:
        torch.softmax = lambda *args, **kw: ps.append(real(*args, **kw)) or ps[-1]
        est = net(x, dyn, torch.zeros(x.shape[0], D, 1, dtype=torch.float64))
    finally:
        torch.softmax = real
    assert est.dtype is torch.float64 and tuple(est.shape) == (x.shape[0], 1)
    (est.view(-1) * a).sum().backward()
    rel = lambda got, want: float(np.abs(got - want).max()) / float(np.abs(want).max())
    assert rel(est.detach().view(-1).numpy(), z["est"]) <= 1e-12
    p = torch.stack([q.squeeze(1) for q in ps], 1).detach().numpy()
    assert p.shape == z["p"].shape and rel(p, z["p"]) <= 1e-12
    for k, v in net.named_parameters():
        w = z["grad_" + k]
        if np.abs(w).max() == 0:
            assert not bool(v.grad.any()), k                                     # (x0 and h0 are zeros)
        else:
            assert rel(v.grad.numpy(), w) <= 1e-12, k
    # decoder_input=None is the zero x0, run for one row
    with torch.no_grad():
        assert float((net(x, dyn) - est).abs().max()) <= 1e-13 * float(est.abs().max())
        # the shadow off the GPU: the torch path on the unpacked bits
        bits = torch.from_numpy(M.pack_bits(z["dynamic"]))
        assert torch.equal(net(x, bits), net(x, dyn))


@pytest.mark.parametrize("S,n,rows,nR,H", [(2, 3, 30, 20, 64), (3, 1, 30, 60, 64), (4, 3, 70, 8, 128)])
def test_fold_through_the_folded_model(S, n, rows, nR, H):
    """StateCritic.fold() handed to critic_model's folded form, float64: the module's torch path to 1e-13 relative"""
    B = 5
    net = _xavier_(tools.StateCritic(S, rows, H, n_process_blocks=n), 10 * S + n).double().eval()
    rng = np.random.RandomState(S + n)
    x = torch.from_numpy(rng.randint(1, 6, size=(B, S, nR)).astype(np.float64))
    dyn = rng.rand(B, rows, nR) < 0.2
    dec = torch.from_numpy(rng.randn(B, S, 1))
    with torch.no_grad():
        f = net.fold()
        assert tuple(f.G.shape) == (3 * H, S) and tuple(f.g.shape) == (3 * H,) and tuple(f.M.shape) == (H, rows)
        assert tuple(f.v.shape) == tuple(f.w2.shape) == (H,) and tuple(f.b2.shape) == (1,)
        for dec_in in (dec, None):
            want = net(x, torch.from_numpy(dyn.astype(np.float64)), dec_in).view(-1)
            q0 = net._rnn_out(x, dec_in, None).matmul(f.Wq.t())
            assert tuple(q0.shape) == ((B, H) if dec_in is not None else (1, H))
            got = M.folded_torch(x, torch.from_numpy(dyn.astype(np.float64)), f.G, f.g, f.M, q0, f.v, f.w2, f.b2, n)[0]
            got_np = M.folded(x.numpy(), dyn, *(t.numpy() for t in (f.G, f.g, f.M, q0, f.v, f.w2, f.b2)), n)[0]
            scale = float(want.abs().max())
            assert float((got - want).abs().max()) <= 1e-13 * scale and float(np.abs(got_np - want.numpy()).max()) <= 1e-13 * scale
    # fold() is differentiable: L through the folded model gives the torch path's gradients
    a = torch.from_numpy(rng.randn(B))
    net.zero_grad()
    (net(x, torch.from_numpy(dyn.astype(np.float64)), dec).view(-1) * a).sum().backward()
    want = {k: v.grad.clone() for k, v in net.named_parameters()}
    net.zero_grad()
    f = net.fold()
    q0 = net._rnn_out(x, dec, None).matmul(f.Wq.t())
    (M.folded_torch(x, torch.from_numpy(dyn.astype(np.float64)), f.G, f.g, f.M, q0, f.v, f.w2, f.b2, n)[0] * a).sum().backward()
    for k, v in net.named_parameters():
        assert float((v.grad - want[k]).abs().max()) <= 1e-12 * max(float(want[k].abs().max()), 1e-300), k


def test_model_forms_agree():
    for rows, nR, H, S, n in ((30, 20, 64, 2, 3), (126, 60, 128, 4, 2), (10, 4, 64, 2, 1)):
        X = M.make_case(3, rows, nR, H, S, n, 0.1, 11 * rows + nR)
        want = M.reference_form(X, np.float64)
        G, g, Mf, q0 = M.fold(X, np.float64)
        got = M.folded(X["x"], X["dyn"], G, g, Mf, q0, X["v"], X["w2"], X["b2"], n, np.float64)
        tt = M.reference_form_torch(X, torch.float64)
        for a, b, w in zip(got, tt, want):
            assert a.shape == w.shape and float(np.abs(a - w).max()) <= 1e-12 and float(np.abs(b.numpy() - w).max()) <= 1e-12
        f = lambda a: np.asarray(a, np.float32)
        f32 = M.folded(X["x"], X["dyn"], f(G), f(g), f(Mf), f(q0), X["v"], X["w2"], X["b2"], n, np.float32)
        assert f32[0].dtype == np.float32 and float(np.abs(f32[0] - want[0]).max()) <= 1e-4


def test_torch_path_takes_over_where_there_is_no_kernel():
    """two GRU layers, nine process blocks, H = 32: all run (on the CPU everything does), float dynamic and shadow alike"""
    rng = np.random.RandomState(5)
    x = torch.from_numpy(rng.randint(1, 6, size=(3, 2, 8)).astype(np.float32))
    dyn = rng.rand(3, 10, 8) < 0.3
    for kw in (dict(num_layers=2), dict(n_process_blocks=9), dict()):
        net = _xavier_(tools.StateCritic(2, 10, 32, **kw), 3).eval()
        with torch.no_grad():
            a, b = net(x, torch.from_numpy(dyn.astype(np.float32))), net(x, torch.from_numpy(M.pack_bits(dyn)))
        assert tuple(a.shape) == (3, 1) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    with pytest.raises(TypeError):
        net(x, torch.zeros(3, 10, 8, dtype=torch.int32))
    # a two-plane shadow (70 rows) unpacks plane 0 before plane 1
    net, dyn = _xavier_(tools.StateCritic(2, 70, 32), 4).eval(), rng.rand(3, 70, 8) < 0.3
    with torch.no_grad():
        assert torch.equal(net(x, torch.from_numpy(dyn.astype(np.float32))), net(x, torch.from_numpy(M.pack_bits(dyn))))


def test_exports_and_signatures():
    L = _lib.lib()
    for name in ("tap_critic_value", "tap_critic_value_backward", "tap_critic_value_backward_scratch"):
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(L, name)
    assert _lib.TAP_HIT_CRITIC == 31 == _lib.TAP_HIT_HEIGHTMAP + 1
    assert list(inspect.signature(T.critic_value).parameters) == ["x", "bits", "G", "g", "M", "q0", "v", "w2", "b2", "blocks", "rows"]
    assert T.rollout.critic_value is T.critic_value and "critic_value" in T.__all__
    assert T.StateCritic is tools.StateCritic and T.realCritic is T.StateCritic and tools.realCritic is tools.StateCritic
    assert "StateCritic" in T.__all__ and "realCritic" in T.__all__
    sig = inspect.signature(T.StateCritic.__init__).parameters
    assert list(sig) == ["self", "static_size", "dynamic_size", "hidden_size", "num_layers", "n_process_blocks", "dropout"]
    assert sig["num_layers"].default == 1 and sig["n_process_blocks"].default == 3 and sig["dropout"].default == 0.2
    assert list(inspect.signature(T.StateCritic.forward).parameters)[:5] == ["self", "static", "dynamic", "decoder_input", "last_hh"]
    assert T.rollout.critic_value_supported(30, 20, 128, 2, 3) and not T.rollout.critic_value_supported(30, 20, 128, 9, 3)
    assert not T.rollout.critic_value_supported(30, 20, 128, 2, 9) and not T.rollout.critic_value_supported(30, 22, 128, 2, 3)
    assert not T.rollout.critic_value_supported(30, 20, 32, 2, 3) and not T.rollout.critic_value_supported(129, 20, 128, 2, 3)


def test_host_side_checks_need_no_device():
    """the argument checks of both entries, in the header's order, with a null context and host addresses that are never
    dereferenced"""
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED
    NF, NB = 14, 12                                                   # buffers of the forward / the backward (scratch apart)

    def fwd(B, nR, rows, H, S=2, n=3, bufs=None, stride=None):
        b = [None] * NF if bufs is None else bufs
        return L.tap_critic_value(None, b[0], b[1], B, nR, rows, H, S, n, b[2], b[3], b[4], b[5], H if stride is None else stride,
                                  *b[6:14], None)

    def bwd(B, nR, rows, H, S=2, n=3, bufs=None, scr=None, nbytes=0):
        b = [None] * NB if bufs is None else bufs
        return L.tap_critic_value_backward(None, b[0], b[1], B, nR, rows, H, S, n, *b[2:12], scr, nbytes, None)
    for f in (fwd, bwd):
        # 1. a negative B or a non-positive dimension, before anything else
        assert f(-1, 20, 30, 128) == inv
        for dims in ((0, 30, 128, 2, 3), (20, 0, 128, 2, 3), (20, 30, 0, 2, 3), (-4, 30, 128, 2, 3), (20, 30, 128, 0, 3), (20, 30, 128, 2, 0)):
            assert f(2, *dims) == inv and f(0, *dims) == inv
        # 2. an empty batch is fine whatever the buffers and the shape are: nothing would run
        assert f(0, 20, 30, 128) == ok and f(0, 22, 30, 128) == ok and f(0, 20, 129, 128) == ok and f(0, 20, 30, 100) == ok
        assert f(0, 20, 30, 128, 9, 3) == ok and f(0, 20, 30, 128, 2, 9) == ok
        # 3. null buffers, before the shape is looked at
        assert f(1, 20, 30, 128) == inv and f(1, 22, 30, 100) == inv
    for hole in range(NF):
        args = [p] * NF
        args[hole] = None
        assert fwd(1, 20, 30, 128, bufs=args) == inv and fwd(1, 22, 30, 100, bufs=args) == inv
    for hole in range(NB):
        args = [p] * NB
        args[hole] = None
        assert bwd(1, 20, 30, 128, bufs=args, scr=p, nbytes=1 << 30) == inv and bwd(1, 22, 30, 100, bufs=args, scr=p, nbytes=1 << 30) == inv
    # 4. shapes without a shadow, hidden sizes without an instantiation, too many static rows or blocks, a q0 stride
    for dims in ((20, 129, 128, 2, 3), (22, 30, 128, 2, 3), (260, 30, 128, 2, 3), (20, 30, 32, 2, 3), (20, 30, 100, 2, 3),
                 (20, 30, 512, 2, 3), (20, 30, 128, 9, 3), (20, 30, 128, 2, 9)):
        assert fwd(2, *dims, bufs=[p] * NF) == uns
        assert bwd(2, *dims, bufs=[p] * NB, scr=p, nbytes=1 << 30) == uns
        assert L.tap_critic_value_backward_scratch(2, *dims) == 0
    assert fwd(2, 20, 30, 128, bufs=[p] * NF, stride=64) == uns and fwd(2, 20, 30, 128, bufs=[p] * NF, stride=-128) == uns
    # 5. the backward's scratch: the query, and a scratch that is too small or missing; then the alignment
    need = L.tap_critic_value_backward_scratch(5, 20, 30, 128, 2, 3)
    assert need == 2 * 128 * 4                                        # one partial of H floats per workgroup of four envs
    assert L.tap_critic_value_backward_scratch(0, 20, 30, 128, 2, 3) == 0
    assert L.tap_critic_value_backward_scratch(8192, 20, 30, 128, 2, 3) <= 1 << 20
    assert bwd(5, 20, 30, 128, bufs=[p] * NB, scr=p, nbytes=need - 1) == inv
    assert bwd(5, 20, 30, 128, bufs=[p] * NB, scr=None, nbytes=need) == inv
    q4, q2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    for hole in range(NF):
        args = [p] * NF
        args[hole] = q4 if hole == 1 else q2                          # the shadow's words are 8 bytes, the rest floats
        assert fwd(1, 20, 30, 128, bufs=args) == inv
    args = [p] * NB
    args[1] = q4
    assert bwd(5, 20, 30, 128, bufs=args, scr=p, nbytes=need) == inv
    assert bwd(5, 20, 30, 128, bufs=[p] * NB, scr=q2, nbytes=need) == inv
    args = [p] * NB
    args[9] = C.c_void_p(p.value + 8)                                 # dU leaves as float4s
    assert bwd(5, 20, 30, 128, bufs=args, scr=p, nbytes=need) == inv


def test_wrapper_shape_and_dtype_errors():
    B, S, nR, H, rows = 3, 2, 20, 64, 30
    z = torch.zeros
    x, bits = z(B, S, nR), z(B, nR, dtype=torch.int64)
    G, g, Mf, q0, v, b2 = z(3 * H, S), z(3 * H), z(H, rows), z(B, H), z(H), z(1)
    with pytest.raises(TypeError):
        T.critic_value(x, bits.to(torch.int32), G, g, Mf, q0, v, v, b2, 3)
    for bad in (z(B, nR), z(B, S, nR, dtype=torch.int64)):
        with pytest.raises(ValueError):
            T.critic_value(bad, bits, G, g, Mf, q0, v, v, b2, 3)
    with pytest.raises(ValueError):
        T.critic_value(x, bits, G, g, Mf, q0, v, v, b2, 3, rows=29)
    with pytest.raises(ValueError):
        T.critic_value(x, bits, G[:-1], g, Mf, q0, v, v, b2, 3)
    with pytest.raises(ValueError):
        T.critic_value(x, bits, G, g, Mf, z(2, H), v, v, b2, 3)
    with pytest.raises(ValueError):
        T.critic_value(x, bits, G, g, Mf, q0, v[:-1], v, b2, 3)
    with pytest.raises(ValueError):
        T.critic_value(x, bits, G, g, Mf, q0, v, v, b2, 9)                          # nine blocks: no kernel
    with pytest.raises(ValueError):
        T.critic_value(x, bits, G, g, z(H, 70), q0, v, v, b2, 3)                    # two planes wanted, one given
    with pytest.raises(ValueError):
        T.critic_value(z(B, S, 22), z(B, 22, dtype=torch.int64), G, g, Mf, q0, v, v, b2, 3)   # no shadow
    # well-formed arguments on the host: refused loudly, there is no CPU path
    with pytest.raises(T.TapError):
        T.critic_value(x, bits, G, g, Mf, q0, v, v, b2, 3)
