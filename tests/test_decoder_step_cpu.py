"""The decoder step without a GPU: the folded model against the reference's form (tests/decoder_step_model.py), the exports,
``tools.Pointer.fold_decoder`` / ``fold_episode`` (values and gradients), the state dict, the C entries' host-side checks
and ``forward_step``'s torch path."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch
from torch import nn

import decoder_step_model as M
import tap_net_amd as T
from tap_net_amd import _lib, rollout, tools

# (Ks, Kd, Hd, combine, identity): the reference's two encoders concatenated, the summed encodings, each single encoder,
# and an encoded dynamic half behind identity columns, concatenated (the 3D case) and summed
FOLDS = [(2, 4, 64, 'cat', 0), (2, 4, 64, 'sum', 0), (3, 0, 64, 'cat', 0), (0, 4, 64, 'cat', 0), (3, 0, 32, 'sum', 0),
         (3, 16, 64, 'cat', 16), (3, 32, 32, 'sum', 32), (3, 77, 64, 'cat', 0)]


@pytest.mark.parametrize("Ks,Kd,Hd,combine,identity", FOLDS)
def test_folded_model_equals_the_reference_form(Ks, Kd, Hd, combine, identity):
    """sums of at most 80 + 64 terms of O(50): 1e-12 is far above 144 * 50 * 2^-53"""
    X = M.make_case(5, Ks, Kd, Hd, 100 * Ks + Kd, combine, identity)
    P, c = M.fold(X)
    assert P.shape == (3 * Hd, Ks + Kd) and c.shape == (3 * Hd,)
    for with_h in (True, False):
        with torch.no_grad():
            want = [w.numpy() for w in M.reference_form_torch(X, torch.float64, with_h)]
        hn, q, gates = M.step(X["xs"], X["xd"], X["h"] if with_h else None, P, c, X["W_hh"], X["b_hh"], X["Wq"])
        assert gates.shape == (5, 4, Hd) and np.abs(want[0]).max() > 0.1
        assert float(np.abs(hn - want[0]).max()) <= 1e-12 and float(np.abs(q - want[1]).max()) <= 1e-12
        t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))
        tt = M.step_torch(*(t(a) for a in (X["xs"], X["xd"], X["h"] if with_h else None, P, c, X["W_hh"], X["b_hh"], X["Wq"])))
        for g, w in zip(tt, (hn, q, gates)):
            assert float(np.abs(g.numpy() - w).max()) <= 1e-12
        # the float32 model is the same function, a float32 away
        f32 = M.step(X["xs"], X["xd"], X["h"] if with_h else None, *(np.asarray(a, np.float32) for a in (P, c)), X["W_hh"],
                     X["b_hh"], X["Wq"], dtype=np.float32)
        assert f32[0].dtype == np.float32 and float(np.abs(f32[0] - hn).max()) <= 1e-3


def test_exports_and_signatures():
    L = _lib.lib()
    for name in ("tap_decoder_step", "tap_decoder_step_backward"):
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(L, name)
    assert _lib.TAP_HIT_DECODER == 29 == _lib.TAP_HIT_POINTER + 1
    assert T.rollout.decoder_step is T.decoder_step and "decoder_step" in T.__all__
    assert list(inspect.signature(T.decoder_step).parameters) == ["xs", "xd", "h", "P", "c", "w_hh", "b_hh", "wq"]
    assert list(inspect.signature(T.Pointer.forward_step).parameters) == [
        "self", "proj", "bits", "fold", "decoder_static", "decoder_dynamic", "last_hh"]
    sup = rollout.decoder_step_supported
    assert sup(2, 4, 64) and sup(0, 4, 128) and sup(3, 0, 256) and sup(3, 77, 64) and sup(16, 256, 256)
    assert not sup(0, 0, 64) and not sup(3, 78, 64) and not sup(2, 4, 96) and not sup(2, 4, 32) and not sup(-1, 4, 64)


def test_host_side_checks_need_no_device():
    """the argument checks of both entries, in the header's order, with a null context and host addresses that are never
    dereferenced"""
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED

    def fwd(B, Ks, Kd, Hd, bufs=None):
        """bufs: xs, xd, h, P, c, w_hh, b_hh, wq, h_out, q_out, gates_out"""
        b = [None] * 11 if bufs is None else bufs
        return L.tap_decoder_step(None, b[0], Ks, b[1], Kd, b[2], B, Hd, *b[3:11], None)

    def bwd(B, Hd, bufs=None):
        """bufs: gates, h, g_h, dgi_out, dghn_out, dh_carry_out"""
        b = [None] * 6 if bufs is None else bufs
        return L.tap_decoder_step_backward(None, B, Hd, *b, None)
    # 1. dimensions, before anything else
    for dims in ((-1, 2, 4, 64), (2, -1, 4, 64), (2, 2, -4, 64), (2, 2, 4, 0), (0, 2, 4, -64)):
        assert fwd(*dims) == inv
    assert bwd(-1, 64) == inv and bwd(2, 0) == inv and bwd(0, -1) == inv
    # 2. an empty batch is fine whatever the buffers and the shape are
    assert fwd(0, 2, 4, 64) == ok and fwd(0, 0, 0, 64) == ok and fwd(0, 2, 4, 96) == ok and bwd(0, 64) == ok and bwd(0, 96) == ok
    # 3. null required buffers, before the shape is looked at; h and gates_out may be null, xs iff Ks == 0, xd iff Kd == 0
    assert fwd(1, 2, 4, 64) == inv and fwd(1, 2, 4, 96) == inv and bwd(1, 64) == inv and bwd(1, 96) == inv
    for hole in range(11):
        args = [p] * 11
        args[hole] = None
        assert fwd(1, 2, 4, 96, args) == (uns if hole in (2, 10) else inv), hole      # (a null h or gates_out passes on to the shape)
        if hole not in (2, 10):
            assert fwd(1, 2, 4, 64, args) == inv, hole
    args = [None, p] + [p] * 9
    assert fwd(1, 0, 4, 96, args) == uns and fwd(1, 1, 4, 96, args) == inv
    args = [p, None] + [p] * 9
    assert fwd(1, 3, 0, 96, args) == uns and fwd(1, 3, 1, 96, args) == inv
    for hole in range(6):
        args = [p] * 6
        args[hole] = None
        assert bwd(1, 96, args) == (uns if hole == 1 else inv), hole
    # 4. the shapes: Hd 64, 128, 256 and 1 <= Ks + Kd <= Hd + 16
    for dims in ((2, 4, 96), (2, 4, 32), (2, 4, 512), (0, 0, 64), (3, 78, 64), (81, 0, 64), (17, 256, 256)):
        assert fwd(2, *dims, [p] * 11) == uns, dims
    assert bwd(2, 96, [p] * 6) == uns and bwd(2, 32, [p] * 6) == uns
    # 5. the alignment: 4 bytes, every buffer
    q2 = C.c_void_p(p.value + 2)
    for hole in range(11):
        args = [p] * 11
        args[hole] = q2
        assert fwd(1, 2, 4, 64, args) == inv, hole
    for hole in range(6):
        args = [p] * 6
        args[hole] = q2
        assert bwd(1, 64, args) == inv, hole


def test_wrapper_shape_errors_and_no_cpu_path():
    B, Hd = 3, 64
    z = torch.zeros
    xs, xd, h = z(B, 2, 1), z(B, 4, 1), z(B, Hd)
    P, c, w, b, wq = z(3 * Hd, 6), z(3 * Hd), z(3 * Hd, Hd), z(3 * Hd), z(Hd, Hd)
    for bad in ((xs, xd, h, z(3 * Hd, 7), c, w, b, wq), (xs, xd, h, P, c[:-1], w, b, wq), (xs, xd, z(B, Hd + 1), P, c, w, b, wq),
                (xs, xd, h, P, c, w, b, z(Hd, Hd + 1)), (None, None, h, P, c, w, b, wq), (xs, z(B + 1, 4), h, P, c, w, b, wq),
                (xs, xd, h, z(3 * 96, 6), z(3 * 96), z(3 * 96, 96), z(3 * 96), z(96, 96)), (xs.long(), xd, h, P, c, w, b, wq)):
        with pytest.raises(ValueError):
            T.decoder_step(*bad)
    with pytest.raises(T.TapError):                                   # well-formed arguments on the host: no CPU path
        T.decoder_step(xs, xd, h, P, c, w, b, wq)


def _pointer(Hd, seed, **kw):
    torch.manual_seed(seed)
    net = tools.Pointer(Hd, Hd, 'shape_heightmap', 'bot', **kw).double()
    for p in net.parameters():
        nn.init.xavier_uniform_(p) if p.dim() > 1 else nn.init.normal_(p, std=0.1)
    return net


@pytest.mark.parametrize("Ks,Kd,Hd,combine,identity", FOLDS)
def test_fold_decoder_equals_the_model(Ks, Kd, Hd, combine, identity):
    X = M.make_case(2, Ks, Kd, Hd, 7 * Ks + Kd, combine, identity)
    enc_s, enc_d, gru = M.reference_modules(X, torch.float64)
    net = _pointer(Hd, 1)
    net.gru.load_state_dict(gru.state_dict())
    with torch.no_grad():
        P, c = net.fold_decoder(enc_s, enc_d, combine=combine, identity_dynamic=identity)
    Pw, cw = M.fold(X)
    assert float(np.abs(P.numpy() - Pw).max()) <= 1e-12 and float(np.abs(c.numpy() - cw).max()) <= 1e-12
    assert P.static_decoder is enc_s and P.dynamic_decoder is enc_d and P.combine == combine and P.identity_dynamic == identity


def test_fold_decoder_takes_every_encoder_form_and_refuses_the_rest():
    net = _pointer(32, 2)

    class Encoder(nn.Module):                                         # the reference's Encoder: a module with a ``conv``
        def __init__(self, i, o):
            super(Encoder, self).__init__()
            self.conv = nn.Conv1d(i, o, kernel_size=1)

        def forward(self, x):
            return self.conv(x)
    a, b = Encoder(2, 16).double(), T.DynamicBitsEncoder(4, 16).double()
    P, c = net.fold_decoder(a, b)
    P2, c2 = net.fold_decoder(a.conv, b.conv)
    assert tuple(P.shape) == (96, 6) and torch.equal(P, P2) and torch.equal(c, c2)
    nobias = nn.Conv1d(2, 32, 1, bias=False).double()
    P3, c3 = net.fold_decoder(nobias)
    assert torch.equal(c3, net.gru.bias_ih_l0) and torch.allclose(P3, net.gru.weight_ih_l0 @ nobias.weight[:, :, 0])
    for bad in (dict(), dict(static_decoder=a), dict(static_decoder=a, dynamic_decoder=b, combine='sum'),
                dict(static_decoder=a, dynamic_decoder=b, combine='mean'), dict(static_decoder=a, dynamic_decoder=b, identity_dynamic=16),
                dict(static_decoder=nn.Conv1d(2, 32, 3).double()), dict(static_decoder=a, identity_dynamic=8)):
        with pytest.raises(ValueError):
            net.fold_decoder(**bad)


def test_folds_are_differentiable():
    """gradcheck in float64 of fold_decoder (both combinations) and fold_episode with respect to every parameter they read"""
    Hd = 4
    net = _pointer(Hd, 3)
    enc_s, enc_d, enc_sum = nn.Conv1d(2, 2, 1).double(), nn.Conv1d(3, 2, 1).double(), nn.Conv1d(3, Hd, 1).double()
    dyn = T.DynamicBitsEncoder(5, Hd).double()

    def run(names, fn):
        mods = dict(net=net, enc_s=enc_s, enc_d=enc_d, enc_sum=enc_sum, dyn=dyn)
        leaves = [(mods[m], n) for m, n in names]
        vals = tuple(dict(mod.named_parameters())[n].detach().clone().requires_grad_(True) for mod, n in leaves)

        def f(*ts):
            keep = []
            for (mod, n), t in zip(leaves, ts):                       # the modules' parameters replaced by the leaves
                owner, attr = mod, n
                while "." in attr:
                    head, attr = attr.split(".", 1)
                    owner = getattr(owner, head)
                keep.append((owner, attr, owner._parameters.pop(attr)))
                setattr(owner, attr, t)
            try:
                return fn()
            finally:
                for owner, attr, p in keep:
                    delattr(owner, attr)
                    owner._parameters[attr] = p
        assert torch.autograd.gradcheck(f, vals)
    gru = [("net", "gru.weight_ih_l0"), ("net", "gru.bias_ih_l0")]
    run(gru + [("enc_s", "weight"), ("enc_s", "bias"), ("enc_d", "weight"), ("enc_d", "bias")],
        lambda: tuple(net.fold_decoder(enc_s, enc_d)))
    run(gru + [("enc_sum", "weight"), ("enc_sum", "bias")],
        lambda: tuple(net.fold_decoder(None, enc_sum, combine='sum')))

    def episode():
        with torch.no_grad():
            P, c = net.fold_decoder(enc_s, enc_d)
        fold = net.fold_episode(dyn, P, c)
        return fold.M, fold.k, fold.Wq
    run([("net", "W"), ("net", "encoder_attn.W"), ("dyn", "conv.weight"), ("dyn", "conv.bias")], episode)
    fold = net.fold_episode(dyn, *net.fold_decoder(enc_s, enc_d))
    assert fold.w_hh is net.gru.weight_hh_l0 and fold.b_hh is net.gru.bias_hh_l0 and fold.w_ih is net.gru.weight_ih_l0
    assert fold.Wq.is_contiguous() and fold.rows == 5 and fold.static_decoder is enc_s and fold.combine == 'cat'
    assert tuple(fold.M.shape) == (3 * Hd, 5) and tuple(fold.k.shape) == (3 * Hd,) and tuple(fold.va.shape) == (Hd,)


def test_state_dict_keys_are_unchanged():
    net = tools.Pointer(32, 32, 'shape_heightmap', 'bot')
    assert sorted(net.state_dict()) == sorted(["W", "v", "encoder_attn.W", "encoder_attn.v", "gru.weight_ih_l0", "gru.weight_hh_l0",
                                               "gru.bias_ih_l0", "gru.bias_hh_l0"])
    assert len(list(net.parameters())) == 8


@pytest.mark.parametrize("combine", ["cat", "sum"])
def test_forward_step_on_the_cpu_is_forward_bits_on_the_unfolded_inputs(combine):
    """float64 on the CPU: no device, so forward_step takes the torch path -- the decoder's encoders, then forward_bits,
    which (Hd = 32 has no kernel) is ``forward`` on the encoder's output; as in test_pointer_cpu the fallback hands ``bits``
    to the encoder as it is, here the floating ``dynamic``"""
    Hd, B, nR = 32, 3, 8
    net = _pointer(Hd, 5).eval()
    enc = T.DynamicBitsEncoder(10, Hd).double()
    o = Hd // 2 if combine == 'cat' else Hd
    dec_s, dec_d = nn.Conv1d(2, o, 1).double(), nn.Conv1d(4, o, 1).double()
    sh, dyn = torch.randn(B, Hd, nR).double(), (torch.rand(B, 10, nR) < 0.3).double()
    ds, dd = torch.randint(0, 6, (B, 2, 1)).double(), torch.randint(0, 51, (B, 4, 1)).double()
    hh = torch.randn(1, B, Hd).double()
    with torch.no_grad():
        proj = net.project_static(sh)
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d, combine=combine))
        hidden = torch.cat((dec_s(ds), dec_d(dd)), 1) if combine == 'cat' else dec_s(ds) + dec_d(dd)
        for last in (hh, None):
            want = net.forward_bits(proj, dyn, enc, hidden, last)
            got = net.forward_step(proj, dyn, fold, ds, dd, last)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and tuple(got[1].shape) == (1, B, Hd)
            # and the folded algebra says the same in float64
            hn, q, _ = M.step_torch(ds[:, :, 0], dd[:, :, 0], None if last is None else last[0], fold.P, fold.c, fold.w_hh,
                                    fold.b_hh, fold.Wq)
            assert float((hn - want[1][0]).abs().max()) <= 1e-12
