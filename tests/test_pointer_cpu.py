"""The pointer network on the bit shadow without a GPU: the module against the reference's recorded outputs
(tests/golden/pointer.npz), its state dict, the numpy model's folded form against its restatement of the reference's
form (tests/pointer_model.py), the exports, and the C entries' host-side checks."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import golden_util
import pointer_model as M
import tap_net_amd as T
from tap_net_amd import _lib, tools

KEYS = ["W", "v", "encoder_attn.W", "encoder_attn.v", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0",
        "gru.bias_hh_l0"]


def _golden():
    z = golden_util.load("pointer.npz")
    for i, case in enumerate(z["cases"]):
        He, Hd = (int(v) for v in str(case).split(","))
        pre = "c%d_" % i
        sd = {k[len(pre) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre + "sd_")}
        rec = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre) and not k.startswith(pre + "sd_")}
        yield He, Hd, sd, rec


def test_fixture_holds_both_cases():
    cases = list(_golden())
    assert [(c[0], c[1]) for c in cases] == [(32, 32), (16, 32)]
    for He, Hd, sd, rec in cases:
        assert tuple(rec["static_hidden"].shape) == (3, He, 8) and tuple(rec["probs"].shape) == (3, 8)
        assert rec["probs"].dtype is torch.float64 and rec["last_hh"].dtype is torch.float64


def test_state_dict_keys_and_strict_load():
    net = tools.Pointer(32, 32, 'shape_heightmap', 'bot')
    assert sorted(net.state_dict()) == sorted(KEYS)
    assert tuple(net.W.shape) == (1, 32, 128) and tuple(net.encoder_attn.W.shape) == (1, 32, 96)
    assert tuple(net.v.shape) == tuple(net.encoder_attn.v.shape) == (1, 1, 32)
    for He, Hd, sd, rec in _golden():
        assert sorted(sd) == sorted(KEYS)
        net = tools.Pointer(He, Hd, 'shape_heightmap', 'bot')
        res = net.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys


def test_forward_equals_the_reference_in_float64():
    """every sum has at most 128 terms of O(1): 128 * 2^-53 is far below 1e-12"""
    for He, Hd, sd, rec in _golden():
        net = tools.Pointer(He, Hd, 'shape_heightmap', 'bot')
        net.load_state_dict(sd, strict=True)
        net = net.double().eval()
        with torch.no_grad():
            probs, last_hh = net(rec["static_hidden"].double(), rec["dynamic_hidden"].double(), rec["decoder_hidden"].double(),
                                 rec["last_hh_in"].double())
        assert probs.dtype is torch.float64 and tuple(probs.shape) == (3, 8)
        assert float((probs - rec["probs"]).abs().max()) <= 1e-12
        assert float((last_hh - rec["last_hh"]).abs().max()) <= 1e-12
        assert float(rec["probs"].abs().max()) > 0.05                 # the recorded values are not degenerate


def test_folded_model_equals_the_reference_form():
    for rows, nR, He, Hd in ((30, 20, 128, 128), (126, 60, 64, 128), (10, 4, 128, 64)):
        X = M.make_case(3, rows, nR, He, Hd, 0.1, 11 * rows + nR)
        want = M.reference_form(X, np.float64)
        proj, Mf, k, q = M.fold(X, np.float64)
        got = M.folded(proj, X["dyn"], Mf, k, q, X["va"], X["vp"], np.float64)
        for g, w in zip(got, want):
            assert g.shape == w.shape and float(np.abs(g - w).max()) <= 1e-12
        assert np.abs(want[0]).max() > 0.1
        # the layout round trip, and the torch restatements in float64
        assert np.array_equal(M.from_layout(M.to_layout(proj)), proj) and M.to_layout(proj).shape == (3, 3, nR, Hd)
        tt = M.reference_form_torch(X, torch.float64)
        for g, w in zip(tt, want):
            assert float(np.abs(g.numpy() - w).max()) <= 1e-12
        c = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        ft = M.folded_torch(c(proj), c(X["dyn"]), c(Mf), c(k), c(q), c(X["va"]), c(X["vp"]))
        for g, w in zip(ft, want):
            assert float(np.abs(g.numpy() - w).max()) <= 1e-12
        # the float32 model is the same function, a float32 away
        f = lambda a: np.asarray(a, np.float32)
        f32 = M.folded(f(proj), X["dyn"], f(Mf), f(k), f(q), X["va"], X["vp"], np.float32)
        assert f32[0].dtype == np.float32 and float(np.abs(f32[0] - want[0]).max()) <= 1e-4


def test_module_folds_like_the_model():
    """project_static, the folded weights and forward_bits' algebra in float64 on the CPU against ``forward``"""
    torch.manual_seed(3)
    He = Hd = 32
    net = tools.Pointer(He, Hd, 'shape_heightmap', 'bot').double().eval()
    for p in net.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    enc = T.DynamicBitsEncoder(10, He).double()
    sh, dyn = torch.randn(3, He, 8).double(), (torch.rand(3, 10, 8) < 0.3).double()
    dec, hh = torch.randn(3, Hd, 1).double(), torch.randn(1, 3, Hd).double()
    with torch.no_grad():
        want, hh2 = net(sh, enc(dyn), dec, hh)
        proj = net.project_static(sh)
        assert tuple(proj.shape) == (3, 3, 8, Hd) and proj.is_contiguous() and proj.static_hidden is sh
        rnn_out, hh3 = net._gru_step(dec, hh)
        Ws, Wd, Wq = net.folded_weights()
        Mf, k = Wd @ enc.conv.weight[:, :, 0], Wd @ enc.conv.bias
        got = M.folded_torch(proj.permute(0, 1, 3, 2).reshape(3, 3 * Hd, 8), dyn, Mf, k, rnn_out @ Wq.t(),
                             net.encoder_attn.v[0, 0], net.v[0, 0])[0]
    assert torch.equal(hh2, hh3) and float((got - want).abs().max()) <= 1e-12


def test_exports_and_signatures():
    L = _lib.lib()
    for name in ("tap_pointer_scores", "tap_pointer_scores_backward", "tap_pointer_scores_backward_scratch"):
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(L, name)
    assert _lib.TAP_HIT_POINTER == 28 == _lib.TAP_HIT_ENCODE_BITS + 1
    assert list(inspect.signature(T.pointer_scores).parameters) == ["proj", "bits", "M", "k", "q", "va", "vp", "rows"]
    assert T.rollout.pointer_scores is T.pointer_scores and "pointer_scores" in T.__all__
    assert T.Pointer is tools.Pointer and "Pointer" in T.__all__
    assert list(inspect.signature(T.Pointer.__init__).parameters) == [
        "self", "encoder_hidden_size", "decoder_hidden_size", "decoder_input_type", "input_type", "num_layers", "dropout"]
    sig = inspect.signature(T.Pointer.__init__).parameters
    assert sig["num_layers"].default == 1 and sig["dropout"].default == 0.2
    assert list(inspect.signature(T.Pointer.forward_bits).parameters) == [
        "self", "proj", "bits", "dynamic_encoder", "decoder_hidden", "last_hh"]


def test_host_side_checks_need_no_device():
    """the argument checks of both entries, in the header's order, with a null context and host addresses that are never
    dereferenced"""
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED

    def fwd(B, nR, rows, Hd, bufs=None):
        b = [None] * 10 if bufs is None else bufs
        return L.tap_pointer_scores(None, b[0], b[1], B, nR, rows, Hd, *b[2:10], None)

    def bwd(B, nR, rows, Hd, bufs=None, scr=None, nbytes=0):
        b = [None] * 14 if bufs is None else bufs
        return L.tap_pointer_scores_backward(None, b[0], b[1], B, nR, rows, Hd, *b[2:14], scr, nbytes, None)
    for f in (fwd, bwd):
        # 1. a negative B or a non-positive dimension, before anything else
        assert f(-1, 20, 30, 128) == inv
        for dims in ((0, 30, 128), (20, 0, 128), (20, 30, 0), (-4, 30, 128)):
            assert f(2, *dims) == inv and f(0, *dims) == inv
        # 2. an empty batch is fine whatever the buffers and the shape are: nothing would run
        assert f(0, 20, 30, 128) == ok and f(0, 22, 30, 128) == ok and f(0, 20, 129, 128) == ok and f(0, 20, 30, 100) == ok
        # 3. null buffers, before the shape is looked at
        assert f(1, 20, 30, 128) == inv and f(1, 22, 30, 100) == inv
    for hole in range(10):
        args = [p] * 10
        args[hole] = None
        assert fwd(1, 20, 30, 128, args) == inv and fwd(1, 22, 30, 100, args) == inv
    for hole in range(14):
        args = [p] * 14
        args[hole] = None
        assert bwd(1, 20, 30, 128, args, p, 1 << 30) == inv and bwd(1, 22, 30, 100, args, p, 1 << 30) == inv
    # 4. shapes without a shadow, and hidden sizes without an instantiation
    for dims in ((20, 129, 128), (22, 30, 128), (260, 30, 128), (20, 30, 32), (20, 30, 100), (20, 30, 512)):
        assert fwd(2, *dims, [p] * 10) == uns
        assert bwd(2, *dims, [p] * 14, p, 1 << 30) == uns
        assert L.tap_pointer_scores_backward_scratch(2, *dims) == 0
    # 5. the backward's scratch: the query, and a scratch that is too small or missing; then the alignment
    need = L.tap_pointer_scores_backward_scratch(3, 20, 30, 128)
    assert need > 0 and need % 4 == 0
    assert L.tap_pointer_scores_backward_scratch(0, 20, 30, 128) == 0
    assert L.tap_pointer_scores_backward_scratch(8192, 20, 30, 128) <= 4 << 20
    assert bwd(3, 20, 30, 128, [p] * 14, p, need - 1) == inv
    assert bwd(3, 20, 30, 128, [p] * 14, None, need) == inv
    q4, q2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    for hole in range(10):
        args = [p] * 10
        args[hole] = q4 if hole == 1 else q2                          # the shadow's words are 8 bytes, the rest floats
        assert fwd(1, 20, 30, 128, args) == inv
    args = [p] * 14
    args[1] = q4
    assert bwd(3, 20, 30, 128, args, p, need) == inv
    assert bwd(3, 20, 30, 128, [p] * 14, q2, need) == inv
    args = [p] * 14
    args[10] = C.c_void_p(p.value + 8)                                # dU leaves as float4s
    assert bwd(3, 20, 30, 128, args, p, need) == inv


def test_wrapper_shape_and_dtype_errors():
    B, nR, Hd, rows = 3, 20, 64, 30
    proj, bits = torch.zeros(B, 3, nR, Hd), torch.zeros(B, nR, dtype=torch.int64)
    Mf, k, q, v = torch.zeros(3 * Hd, rows), torch.zeros(3 * Hd), torch.zeros(B, Hd), torch.zeros(Hd)
    with pytest.raises(TypeError):
        T.pointer_scores(proj, bits.to(torch.int32), Mf, k, q, v, v)
    for bad in (torch.zeros(B, 3 * Hd, nR), torch.zeros(B, 2, nR, Hd), torch.zeros(B, 3, nR, Hd, dtype=torch.int64)):
        with pytest.raises(ValueError):
            T.pointer_scores(bad, bits, Mf, k, q, v, v)
    with pytest.raises(ValueError):
        T.pointer_scores(proj, bits, Mf, k, q, v, v, rows=29)
    with pytest.raises(ValueError):
        T.pointer_scores(proj, bits, Mf[:-1], k, q, v, v)
    with pytest.raises(ValueError):
        T.pointer_scores(proj, bits, Mf, k, q[:, :-1], v, v)
    with pytest.raises(ValueError):
        T.pointer_scores(proj, bits, Mf, k, q, v[:-1], v)
    with pytest.raises(ValueError):
        T.pointer_scores(proj, bits, torch.zeros(3 * Hd, 70), k, q, v, v)          # two planes wanted, one given
    with pytest.raises(ValueError):
        T.pointer_scores(torch.zeros(B, 3, nR, 32), bits, torch.zeros(96, rows), torch.zeros(96), torch.zeros(B, 32),
                         torch.zeros(32), torch.zeros(32))                        # Hd 32: no kernel
    with pytest.raises(ValueError):
        T.pointer_scores(torch.zeros(B, 3, 22, Hd), torch.zeros(B, 22, dtype=torch.int64), Mf, k, q, v, v)   # no shadow
    # well-formed arguments on the host: refused loudly, there is no CPU path
    with pytest.raises(T.TapError):
        T.pointer_scores(proj, bits, Mf, k, q, v, v)


def test_forward_bits_falls_back_on_a_shape_without_a_kernel():
    """Hd = 32 has no kernel: forward_bits is ``forward`` on the encoder's output (here the float path of the encoder:
    the fallback hands ``bits`` to the encoder as it is)"""
    torch.manual_seed(8)
    net = tools.Pointer(32, 32, 'shape_heightmap', 'bot').eval()
    for p in net.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    enc = T.DynamicBitsEncoder(10, 32)
    sh, dyn = torch.randn(3, 32, 8), (torch.rand(3, 10, 8) < 0.3).float()
    dec, hh = torch.randn(3, 32, 1), torch.randn(1, 3, 32)
    with torch.no_grad():
        want = net(sh, enc(dyn), dec, hh)
        got = net.forward_bits(net.project_static(sh), dyn, enc, dec, hh)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError):
        net.forward_bits(torch.zeros(3, 3, 8, 32), dyn, enc, dec, hh)
