"""The 3D decoder step without a GPU: the numpy model (tests/heightmap_model.py) and ``tools.HeightmapEncoder`` against the
reference module's recorded outputs (tests/golden/heightmap_encoder.npz), the exports, the C entry's host-side checks,
``decoder_step_heightmap_supported``, ``tools.Pointer.fold_decoder`` with a height-map encoder (values and gradients),
``forward_step``'s torch path and the wrapper's argument errors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch
from torch import nn

import decoder_step_model as DM
import heightmap_model as HM
import tap_net_amd as T
from tap_net_amd import _lib, rollout, tools

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heightmap_encoder.npz"))
KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias")


def _golden_cases():
    """-> [(name, (C, hidden, W, L), [w1, b1, w2, b2, w3, b3], x (n, C, W, L) float32, out (n, hidden) float64)]: the shipped
    3D actor's encoder on the recorded episode's 640 height maps, then the seeded modules"""
    feats = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "episode_3d.npz"))["features"]
    out = [("pretrained", (2, 128, 5, 5), [GOLDEN["pre_" + k] for k in KEYS], feats.reshape(640, 2, 5, 5).astype(np.float32),
            GOLDEN["pre_out"])]
    for i, case in enumerate(GOLDEN["cases"]):
        shape = tuple(int(v) for v in str(case).split(","))
        out.append(("c%d" % i, shape, [GOLDEN["c%d_sd_%s" % (i, k)] for k in KEYS], GOLDEN["c%d_x" % i], GOLDEN["c%d_out" % i]))
    return out


def test_fixture_holds_what_the_tests_need():
    cases = _golden_cases()
    assert [c[1] for c in cases] == [(2, 128, 5, 5), (1, 64, 5, 5), (4, 64, 5, 5), (2, 64, 10, 10), (1, 32, 4, 12), (2, 32, 5, 6)]
    assert sorted(k for k in GOLDEN.files if k.startswith("pre_")) == sorted(["pre_" + k for k in KEYS] + ["pre_out"])
    for name, (Cc, hidden, W, L), w, x, out in cases:
        assert x.dtype == np.float32 and out.dtype == np.float64 and out.shape == (x.shape[0], hidden) and x.shape[1:] == (Cc, W, L)
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 50 and all(a.dtype == np.float32 for a in w)
        assert tuple(w[4].shape) == (hidden, hidden // 2, (W + 3) // 4, (L + 3) // 4)


def test_model_equals_the_reference_module():
    """sums of at most 288 terms of O(100): 1e-12 is far above 288 * 100 * 2^-53"""
    for name, shape, w, x, out in _golden_cases():
        enc, z1, z2 = HM.encode(x, w)
        assert enc.dtype == np.float64 and np.abs(out).max() > 0.1
        assert float(np.abs(enc - out).max()) <= 1e-12, name
        assert (z1 > 0).any() and (z1 < 0).any() and (z2 > 0).any() and (z2 < 0).any(), name      # both branches of both leaky-ReLUs
        with torch.no_grad():
            tt = HM.encode_torch(torch.from_numpy(x).double(), [torch.from_numpy(a).double() for a in w]).numpy()
        assert float(np.abs(tt - out).max()) <= 1e-12, name
        f32 = HM.encode(x, w, dtype=np.float32)[0]
        assert f32.dtype == np.float32 and float(np.abs(f32 - out).max()) <= 1e-3 * max(1.0, float(np.abs(out).max()))


def test_heightmap_encoder_loads_the_checkpoint_keys_strictly():
    for name, (Cc, hidden, W, L), w, x, out in _golden_cases():
        net = tools.HeightmapEncoder(Cc, hidden, (W, L))
        assert [n for n, _ in net.named_children()] == ["conv1", "conv2", "conv3"] and sorted(net.state_dict()) == sorted(KEYS)
        net.load_state_dict({k: torch.from_numpy(a) for k, a in zip(KEYS, w)}, strict=True)
        with torch.no_grad():
            got = net.double()(torch.from_numpy(x).double())
        assert tuple(got.shape) == (x.shape[0], hidden, 1)
        assert float(np.abs(got[:, :, 0].numpy() - out).max()) <= 1e-12, name
    assert list(inspect.signature(tools.HeightmapEncoder.__init__).parameters) == ["self", "input_size", "hidden_size", "map_size"]
    with torch.no_grad():                                             # the module's own dtype: float32 as constructed
        y = tools.HeightmapEncoder(2, 32, (5, 5))(torch.zeros(2, 2, 5, 5))
    assert y.dtype is torch.float32 and tuple(y.shape) == (2, 32, 1)


def test_exports_and_signatures():
    L = _lib.lib()
    assert "tap_decoder_step_hm" in _lib.EXPORTS and "tap_decoder_step_hm" in _lib._PROTOS and hasattr(L, "tap_decoder_step_hm")
    assert len(_lib._PROTOS["tap_decoder_step_hm"][1]) == 27
    assert _lib.TAP_HIT_HEIGHTMAP == 30 == _lib.TAP_HIT_DECODER + 1
    assert T.HeightmapEncoder is tools.HeightmapEncoder and "HeightmapEncoder" in T.__all__
    assert T.rollout.decoder_step_heightmap is T.decoder_step_heightmap and "decoder_step_heightmap" in T.__all__
    assert list(inspect.signature(T.decoder_step_heightmap).parameters) == ["xs", "hm", "h", "encoder", "P", "c", "w_hh", "b_hh", "wq"]
    assert list(inspect.signature(rollout.decoder_step_heightmap_supported).parameters) == ["Ks", "C", "W", "L", "m", "Hd"]
    assert "heightmap" in tools.StepFold.__slots__


def test_supported_on_both_sides_of_every_bound():
    sup = rollout.decoder_step_heightmap_supported
    assert sup(3, 2, 5, 5, 128, 256) and sup(3, 2, 5, 5, 32, 64) and sup(0, 1, 5, 5, 64, 64) and sup(4, 4, 5, 5, 64, 128)
    # Hd 64, 128, 256 and m = Hd / 2 or Hd
    for Hd in (64, 128, 256):
        assert sup(3, 2, 5, 5, Hd // 2, Hd) and sup(3, 2, 5, 5, Hd, Hd) and not sup(3, 2, 5, 5, Hd // 4, Hd) and not sup(3, 2, 5, 5, 2 * Hd, Hd)
    assert not sup(3, 2, 5, 5, 16, 32) and not sup(3, 2, 5, 5, 256, 512) and not sup(3, 2, 5, 5, 48, 96) and not sup(3, 2, 5, 5, 33, 64)
    # C 1, 2 or 4
    assert [sup(3, Cc, 5, 5, 32, 64) for Cc in (0, 1, 2, 3, 4, 5, 8)] == [False, True, True, False, True, False, False]
    # 1 <= W, L <= 12
    assert sup(3, 2, 1, 1, 32, 64) and sup(3, 2, 12, 12, 32, 64) and sup(3, 2, 1, 12, 32, 64)
    assert not sup(3, 2, 0, 5, 32, 64) and not sup(3, 2, 5, 0, 32, 64) and not sup(3, 2, 13, 5, 32, 64) and not sup(3, 2, 5, 13, 32, 64)
    # 0 <= Ks <= 16 and Ks + m <= Hd + 16
    assert sup(0, 2, 5, 5, 32, 64) and sup(16, 2, 5, 5, 32, 64) and not sup(17, 2, 5, 5, 32, 64) and not sup(-1, 2, 5, 5, 32, 64)
    assert sup(16, 2, 5, 5, 64, 64) and not sup(17, 2, 5, 5, 64, 64) and sup(16, 2, 5, 5, 256, 256) and not sup(17, 2, 5, 5, 128, 256)


def test_host_side_checks_need_no_device():
    """the entry's argument checks in the header's order, with a null context and host addresses that are never
    dereferenced (no call here has every argument valid)"""
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED
    NB, OPTIONAL = 18, (2, 16, 17)          # xs, hm, h, w1, b1, w2, b2, w3, b3, P, c, w_hh, b_hh, wq, h_out, q_out, gates_out, enc_out

    def call(B, Ks, Cc, W, Lh, m, Hd, bufs=None):
        b = [None] * NB if bufs is None else bufs
        return L.tap_decoder_step_hm(None, b[0], Ks, b[1], Cc, W, Lh, b[2], B, Hd, m, *b[3:NB], None)
    good = (3, 2, 5, 5, 32, 64)             # Ks, C, W, L, m, Hd
    # 1. dimensions, before anything else
    for dims in ((-1,) + good, (2, -1, 2, 5, 5, 32, 64), (2, 3, 0, 5, 5, 32, 64), (2, 3, 2, 0, 5, 32, 64), (2, 3, 2, 5, 0, 32, 64),
                 (2, 3, 2, 5, 5, 0, 64), (2, 3, 2, 5, 5, 32, 0), (0, 3, 2, 5, 5, 32, -64), (0, 3, -2, 5, 5, 32, 64)):
        assert call(*dims) == inv, dims
    # 2. an empty batch is fine whatever the buffers and the shape are
    assert call(0, *good) == ok and call(0, 3, 3, 5, 5, 32, 64) == ok and call(0, 3, 2, 13, 5, 32, 96) == ok
    # 3. null required buffers, before the shape is looked at; h, gates_out and enc_out may be null, xs iff Ks == 0
    bad_shape = (3, 2, 5, 5, 32, 96)
    assert call(1, *good) == inv and call(1, *bad_shape) == inv
    for hole in range(NB):
        args = [p] * NB
        args[hole] = None
        assert call(1, *bad_shape, args) == (uns if hole in OPTIONAL else inv), hole      # (an optional null passes on to the shape)
        if hole not in OPTIONAL:
            assert call(1, *good, args) == inv, hole
    args = [None] + [p] * (NB - 1)
    assert call(1, 0, 2, 5, 5, 32, 96, args) == uns and call(1, 1, 2, 5, 5, 32, 96, args) == inv
    # 4. the shapes
    for dims in ((3, 2, 5, 5, 32, 96), (3, 2, 5, 5, 16, 32), (3, 2, 5, 5, 256, 512), (3, 2, 5, 5, 16, 64), (3, 2, 5, 5, 128, 64),
                 (3, 3, 5, 5, 32, 64), (3, 8, 5, 5, 32, 64), (3, 2, 13, 5, 32, 64), (3, 2, 5, 13, 32, 64), (17, 2, 5, 5, 32, 64),
                 (17, 2, 5, 5, 64, 64), (17, 2, 5, 5, 128, 256)):
        assert call(2, *dims, [p] * NB) == uns, dims
    # 5. the alignment: 4 bytes, every buffer
    q2 = C.c_void_p(p.value + 2)
    for hole in range(NB):
        args = [p] * NB
        args[hole] = q2
        assert call(1, *good, args) == inv, hole
        assert call(1, 16, 1, 12, 12, 256, 256, args) == inv, hole                         # every bound of the list at once


def _pointer(Hd, seed, **kw):
    torch.manual_seed(seed)
    net = tools.Pointer(Hd, Hd, 'shape_heightmap', 'bot', **kw).double()
    for p in net.parameters():
        nn.init.xavier_uniform_(p) if p.dim() > 1 else nn.init.normal_(p, std=0.1)
    return net


def _modules(X, dtype=torch.float64):
    """the case's static nn.Conv1d (or None), tools.HeightmapEncoder and nn.GRU, holding its weights"""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)                               # noqa: E731
    enc_s = None
    if X["Ks"]:
        enc_s = nn.Conv1d(X["Ks"], X["os"], 1).to(dtype)
        with torch.no_grad():
            enc_s.weight.copy_(t(X["Ws"])[:, :, None])
            enc_s.bias.copy_(t(X["bs"]))
    enc_d = tools.HeightmapEncoder(X["C"], X["m"], (X["W"], X["L"])).to(dtype)
    enc_d.load_state_dict({k: t(a) for k, a in zip(KEYS, X["enc"])}, strict=True)
    gru = nn.GRU(X["Hd"], X["Hd"], 1, batch_first=True).to(dtype)
    with torch.no_grad():
        for name in ("W_ih", "W_hh", "b_ih", "b_hh"):
            getattr(gru, {"W": "weight", "b": "bias"}[name[0]] + name[1:] + "_l0").copy_(t(X[name]))
    return enc_s, enc_d, gru


# (Ks, C, W, L, m, Hd, combine): the 3D actor's cat, the summed encodings, the height map alone
FOLDS = [(3, 2, 5, 5, 32, 64, 'cat'), (3, 2, 5, 5, 64, 64, 'sum'), (0, 1, 5, 6, 64, 64, 'cat'), (4, 4, 10, 10, 16, 32, 'cat')]


@pytest.mark.parametrize("Ks,Cc,W,L,m,Hd,combine", FOLDS)
def test_fold_decoder_equals_the_model(Ks, Cc, W, L, m, Hd, combine):
    X = HM.make_case(3, Ks, Cc, W, L, m, Hd, 11 * Ks + m, combine)
    enc_s, enc_d, gru = _modules(X)
    net = _pointer(Hd, 1)
    net.gru.load_state_dict(gru.state_dict())
    with torch.no_grad():
        P, c = net.fold_decoder(enc_s, enc_d, combine=combine)
    Pw, cw = HM.fold(X)
    assert tuple(P.shape) == (3 * Hd, Ks + m)
    assert float(np.abs(P.numpy() - Pw).max()) <= 1e-12 and float(np.abs(c.numpy() - cw).max()) <= 1e-12
    assert P.static_decoder is enc_s and P.dynamic_decoder is enc_d and P.combine == combine and P.identity_dynamic == 0
    # the folded model is the reference's form: conv3's bias lives in enc, not in c
    for with_h in (True, False):
        with torch.no_grad():
            want = [w.numpy() for w in HM.reference_form_torch(X, torch.float64, with_h)]
        hn, q, gates, enc = HM.step(X["xs"], X["hm"], X["h"] if with_h else None, X["enc"], Pw, cw, X["W_hh"], X["b_hh"], X["Wq"])
        assert float(np.abs(hn - want[0]).max()) <= 1e-12 and float(np.abs(q - want[1]).max()) <= 1e-12
        assert float(np.abs(enc - want[2]).max()) <= 1e-12
    fold = net.fold_episode(T.DynamicBitsEncoder(5, Hd).double(), P, c)
    assert fold.heightmap is enc_d and fold.dynamic_decoder is enc_d and fold.identity_dynamic == 0
    fold2 = net.fold_episode(T.DynamicBitsEncoder(5, Hd).double(), *net.fold_decoder(nn.Conv1d(Hd, Hd, 1).double()))
    assert fold2.heightmap is None


def test_fold_decoder_refusals_stay():
    net = _pointer(32, 2)
    hm = tools.HeightmapEncoder(2, 16, (5, 5)).double()
    a = nn.Conv1d(3, 16, 1).double()
    assert tuple(net.fold_decoder(a, hm)[0].shape) == (96, 3 + 16)
    assert tuple(net.fold_decoder(None, tools.HeightmapEncoder(2, 32, (5, 5)).double())[0].shape) == (96, 32)
    for bad in (dict(static_decoder=a, dynamic_decoder=hm, identity_dynamic=16), dict(static_decoder=a, dynamic_decoder=hm, combine='sum'),
                dict(static_decoder=a, dynamic_decoder=tools.HeightmapEncoder(2, 32, (5, 5)).double()),
                dict(static_decoder=a, dynamic_decoder=hm, combine='mean'), dict(static_decoder=nn.Conv1d(2, 32, 3).double()),
                dict(static_decoder=a, dynamic_decoder=nn.Conv2d(2, 16, 1).double())):
        with pytest.raises(ValueError):
            net.fold_decoder(**bad)


def test_fold_with_a_heightmap_encoder_is_differentiable():
    """gradcheck in float64 of fold_decoder with respect to what it reads: the GRU's input weights and the static encoder
    (the height-map encoder's parameters do not enter the fold)"""
    Hd = 8
    net = _pointer(Hd, 3)
    enc_s, hm = nn.Conv1d(3, 4, 1).double(), tools.HeightmapEncoder(2, 4, (5, 5)).double()
    names = [(net, "gru.weight_ih_l0"), (net, "gru.bias_ih_l0"), (enc_s, "weight"), (enc_s, "bias")]
    vals = tuple(dict(mod.named_parameters())[n].detach().clone().requires_grad_(True) for mod, n in names)

    def f(*ts):
        keep = []
        for (mod, n), t in zip(names, ts):
            owner, attr = mod, n
            while "." in attr:
                head, attr = attr.split(".", 1)
                owner = getattr(owner, head)
            keep.append((owner, attr, owner._parameters.pop(attr)))
            setattr(owner, attr, t)
        try:
            return tuple(net.fold_decoder(enc_s, hm))
        finally:
            for owner, attr, p in keep:
                delattr(owner, attr)
                owner._parameters[attr] = p
    assert torch.autograd.gradcheck(f, vals)
    P, c = net.fold_decoder(enc_s, hm)
    assert all(p.grad is None for p in hm.parameters()) and not any(p is P for p in hm.parameters())


@pytest.mark.parametrize("combine", ["cat", "sum"])
def test_forward_step_on_the_cpu_is_the_unfolded_reference_form(combine):
    """float64 on the CPU: forward_step takes the torch path, which hands the encoder the 4-D decoder_dynamic; the result is
    forward_bits on the reference's decoder_hidden, and the folded algebra says the same"""
    Hd, B, nR = 32, 3, 8
    m = Hd // 2 if combine == 'cat' else Hd
    net = _pointer(Hd, 5).eval()
    enc = T.DynamicBitsEncoder(10, Hd).double()
    dec_s, dec_d = nn.Conv1d(3, Hd - m if combine == 'cat' else Hd, 1).double(), tools.HeightmapEncoder(2, m, (5, 5)).double()
    sh, dyn = torch.randn(B, Hd, nR).double(), (torch.rand(B, 10, nR) < 0.3).double()
    ds, dd = torch.randint(0, 6, (B, 3, 1)).double(), torch.randint(-50, 51, (B, 2, 5, 5)).double()
    hh = torch.randn(1, B, Hd).double()
    with torch.no_grad():
        proj = net.project_static(sh)
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d, combine=combine))
        hidden = torch.cat((dec_s(ds), dec_d(dd)), 1) if combine == 'cat' else dec_s(ds) + dec_d(dd)
        assert tuple(hidden.shape) == (B, Hd, 1)
        for last in (hh, None):
            want = net.forward_bits(proj, dyn, enc, hidden, last)
            got = net.forward_step(proj, dyn, fold, ds, dd, last)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and tuple(got[1].shape) == (1, B, Hd)
            hn, q, _ = DM.step_torch(ds[:, :, 0], dec_d(dd)[:, :, 0], None if last is None else last[0], fold.P, fold.c, fold.w_hh,
                                     fold.b_hh, fold.Wq)
            assert float((hn - want[1][0]).abs().max()) <= 1e-12


def test_wrapper_shape_errors_and_no_cpu_path():
    B, Hd, m = 3, 64, 32
    z = torch.zeros
    enc = tools.HeightmapEncoder(2, m, (5, 5))
    xs, hm, h = z(B, 3, 1), z(B, 2, 5, 5), z(B, Hd)
    P, c, w, b, wq = z(3 * Hd, 3 + m), z(3 * Hd), z(3 * Hd, Hd), z(3 * Hd), z(Hd, Hd)

    class NoBias(nn.Module):
        def __init__(self):
            super(NoBias, self).__init__()
            self.conv1, self.conv2 = nn.Conv2d(2, 8, 1, stride=2), nn.Conv2d(8, 16, 1, stride=2)
            self.conv3 = nn.Conv2d(16, 32, 2, bias=False)
    for bad in ((xs, hm, h, enc, z(3 * Hd, 4 + m), c, w, b, wq),                       # P's columns
                (xs, hm, h, enc, P, c[:-1], w, b, wq), (xs, hm, z(B, Hd + 1), enc, P, c, w, b, wq), (xs, hm, h, enc, P, c, w, b, z(Hd, Hd + 1)),
                (xs, None, h, enc, P, c, w, b, wq), (xs, z(B, 50, 1), h, enc, P, c, w, b, wq),    # hm must be 4-D
                (z(B + 1, 3), hm, h, enc, P, c, w, b, wq), (xs.long(), hm, h, enc, P, c, w, b, wq), (xs, hm.long(), h, enc, P, c, w, b, wq),
                (xs, z(B, 1, 5, 5), h, enc, P, c, w, b, wq),                               # conv1 takes 2 planes
                (xs, z(B, 2, 10, 10), h, enc, P, c, w, b, wq),                             # conv3's kernel is for a 5 x 5 map
                (xs, hm, h, nn.Conv1d(50, m, 1), P, c, w, b, wq), (xs, hm, h, NoBias(), P, c, w, b, wq),
                (xs, z(B, 2, 13, 5), h, tools.HeightmapEncoder(2, m, (13, 5)), P, c, w, b, wq),   # W > 12: no kernel
                (xs, z(B, 3, 5, 5), h, tools.HeightmapEncoder(3, m, (5, 5)), P, c, w, b, wq),     # C = 3: no kernel
                (xs, hm, h, tools.HeightmapEncoder(2, 16, (5, 5)), z(3 * Hd, 3 + 16), c, w, b, wq),   # m = Hd / 4: no kernel
                (xs, hm, z(B, 96), enc, z(3 * 96, 3 + m), z(3 * 96), z(3 * 96, 96), z(3 * 96), z(96, 96))):
        with pytest.raises(ValueError):
            T.decoder_step_heightmap(*bad)
    with pytest.raises(T.TapError):                                   # well-formed arguments on the host: no CPU path
        T.decoder_step_heightmap(xs, hm, h, enc, P, c, w, b, wq)
