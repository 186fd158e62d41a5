"""The dynamic encoder on the bit shadow without a GPU: the exports, the C entries' host-side checks, the Python
wrapper's shape / dtype errors, the module's state dict and float path, and the numpy model
(tests/dyn_encoder_model.py) against a float64 einsum."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import dyn_encoder_model as M
import tap_net_amd as T
from tap_net_amd import _lib, tools


def test_exports_and_signatures():
    L = _lib.lib()
    for name in ("tap_encode_bits", "tap_encode_bits_backward", "tap_encode_bits_backward_scratch"):
        assert name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(L, name)
    assert L.tap_abi_version() == 1
    assert _lib.TAP_HIT_ENCODE_BITS == 27 == _lib.TAP_HIT_POLICY_PICK + 1
    assert list(inspect.signature(T.encode_dynamic_bits).parameters) == ["bits", "weight", "bias", "rows"]
    assert T.rollout.encode_dynamic_bits is T.encode_dynamic_bits and "encode_dynamic_bits" in T.__all__
    assert T.DynamicBitsEncoder is tools.DynamicBitsEncoder and "DynamicBitsEncoder" in T.__all__
    assert list(inspect.signature(T.DynamicBitsEncoder.__init__).parameters) == ["self", "rows", "hidden_size"]


def test_host_side_checks_need_no_device():
    """the argument checks of both entries, in the header's order, with a null context and null buffers"""
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)                  # a 16-byte aligned host address: never dereferenced here
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED
    fwd = lambda B, nR, rows, H, bits=None, w=None, out=None: L.tap_encode_bits(None, bits, B, nR, rows, H, w, None, out, None)
    bwd = lambda B, nR, rows, H, bits=None, g=None, dw=None, scr=None, nbytes=0: \
        L.tap_encode_bits_backward(None, bits, g, B, nR, rows, H, dw, None, scr, nbytes, None)
    for f in (fwd, bwd):
        # 1. a negative B or a non-positive dimension, before anything else
        assert f(-1, 20, 30, 8) == inv
        for dims in ((0, 30, 8), (20, 0, 8), (20, 30, 0), (-4, 30, 8)):
            assert f(2, *dims) == inv and f(0, *dims) == inv
        # 2. an empty batch is fine whatever the buffers are -- and whatever the shape is: nothing would run
        assert f(0, 20, 30, 8) == ok and f(0, 256, 128, 1024) == ok and f(0, 4, 1, 1) == ok
        assert f(0, 22, 30, 8) == ok and f(0, 20, 129, 8) == ok
        # 3. null buffers, before the shape is looked at
        assert f(1, 20, 30, 8) == inv and f(1, 22, 30, 8) == inv
    for hole in range(3):
        args = [p, p, p]
        args[hole] = None
        assert fwd(1, 20, 30, 8, *args) == inv
        assert bwd(1, 20, 30, 8, *args, scr=p, nbytes=1 << 30) == inv
    # 4. shapes without a shadow, and hidden sizes beyond 1024
    for dims in ((20, 129, 8), (22, 30, 8), (260, 30, 8), (20, 30, 1025)):
        assert fwd(2, *dims, p, p, p) == uns
        assert bwd(2, *dims, p, p, p, p, 1 << 30) == uns
    # the backward's scratch: the query, and a scratch that is too small or missing
    need = L.tap_encode_bits_backward_scratch(3, 20, 30, 8)
    assert need > 0 and need % 4 == 0
    assert L.tap_encode_bits_backward_scratch(3, 22, 30, 8) == 0 and L.tap_encode_bits_backward_scratch(3, 20, 129, 8) == 0
    assert L.tap_encode_bits_backward_scratch(8192, 20, 30, 128) <= 64 << 20
    assert bwd(3, 20, 30, 8, p, p, p, p, need - 1) == inv
    assert bwd(3, 20, 30, 8, p, p, p, None, need) == inv
    # 5. misaligned buffers: the words are 8 bytes, out and g move as float4s, the scratch holds floats
    q4, q8, q2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 8), C.c_void_p(p.value + 2)
    assert fwd(1, 20, 30, 8, q4, p, p) == inv and fwd(1, 20, 30, 8, p, p, q8) == inv
    assert bwd(3, 20, 30, 8, q4, p, p, p, need) == inv and bwd(3, 20, 30, 8, p, q8, p, p, need) == inv
    assert bwd(3, 20, 30, 8, p, p, p, q2, need) == inv


def test_wrapper_shape_and_dtype_errors():
    bits = torch.zeros(3, 20, dtype=torch.int64)
    W = torch.zeros(8, 30)
    with pytest.raises(TypeError):
        T.encode_dynamic_bits(bits.to(torch.int32), W)
    with pytest.raises(TypeError):
        T.encode_dynamic_bits(bits.float(), W)
    for bad_w in (torch.zeros(8), torch.zeros(8, 30, 2), torch.zeros(8, 30, dtype=torch.int64)):
        with pytest.raises(ValueError):
            T.encode_dynamic_bits(bits, bad_w)
    with pytest.raises(ValueError):
        T.encode_dynamic_bits(bits, W, rows=29)                   # rows must be the weight's
    with pytest.raises(ValueError):
        T.encode_dynamic_bits(bits, torch.zeros(8, 70))           # 70 rows: two planes, 20 words are not 2 * nR with nR % 4 == 0
    with pytest.raises(ValueError):
        T.encode_dynamic_bits(torch.zeros(3, 22, dtype=torch.int64), W)           # nR % 4 != 0: no shadow
    with pytest.raises(ValueError):
        T.encode_dynamic_bits(torch.zeros(3, 2, 20, dtype=torch.int64), W)        # two planes given, one expected
    with pytest.raises(ValueError):
        T.encode_dynamic_bits(bits, torch.zeros(1025, 30))
    with pytest.raises(ValueError):
        T.encode_dynamic_bits(bits, W, bias=torch.zeros(7))
    with pytest.raises(ValueError):
        T.encode_dynamic_bits(bits, W, bias=torch.zeros(8, dtype=torch.int64))
    # well-formed arguments on the host: refused loudly, there is no CPU path
    with pytest.raises(T.TapError):
        T.encode_dynamic_bits(bits, W.view(8, 30, 1), bias=torch.zeros(8))


def test_module_loads_the_reference_encoders_state_dict():
    class Encoder(nn.Module):                                      # the shape of the reference's encoder: one child, `conv`
        def __init__(self, input_size, hidden_size):
            super(Encoder, self).__init__()
            self.conv = nn.Conv1d(input_size, hidden_size, kernel_size=1)

    torch.manual_seed(5)
    ref = Encoder(30, 16)
    assert sorted(ref.state_dict()) == ["conv.bias", "conv.weight"]
    enc = T.DynamicBitsEncoder(30, 16)
    assert [n for n, _ in enc.named_children()] == ["conv"]
    res = enc.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    x = (torch.rand(4, 30, 20) < 0.3).float()
    assert torch.equal(enc(x), F.conv1d(x, ref.conv.weight, ref.conv.bias))
    assert torch.equal(enc(x), F.conv1d(x, enc.conv.weight, enc.conv.bias))
    with pytest.raises(TypeError):
        enc(torch.zeros(4, 20, dtype=torch.int32))


def test_model_layout_round_trip():
    for rows, nR in ((10, 4), (64, 8), (65, 8), (128, 12)):
        dyn = np.random.RandomState(rows).rand(3, rows, nR) < 0.4
        bits = M.pack_bits(dyn)
        assert bits.shape == (3, M.planes_of(rows) * nR) and bits.dtype == np.int64
        assert np.array_equal(M.unpack_bits(bits, rows, nR), dyn)
        junk = M.garbage(bits, rows, nR, 1)
        assert np.array_equal(M.unpack_bits(junk, rows, nR), dyn)
        assert rows % 64 == 0 or not np.array_equal(junk, bits)
    # bit r of word c is dynamic[b, r, c]; plane 1 starts at row 64
    dyn = np.zeros((1, 66, 4), bool)
    dyn[0, 3, 1] = dyn[0, 65, 2] = True
    assert M.pack_bits(dyn).tolist() == [[0, 8, 0, 0, 0, 0, 2, 0]]


def test_model_against_float64():
    """The fp32 model is a sequential sum s_0 = bias, s_k = fl(s_{k-1} + t_k) of n = rows terms (unset rows add an exact
    0).  Each addition commits a relative error of at most u = 2^-24 on its result: fl(a + b) = (a + b)(1 + d), |d| <= u.
    Unrolling, term t_k is multiplied by at most (1 + u)^(n - k + 1), so |s_n - sum t| <= ((1 + u)^n - 1) sum |t| =
    n u sum |t| + O(u^2) -- the standard bound for n sequential additions (Higham, Accuracy and Stability, eq. 4.4);
    the second-order part is below 1e-5 of the first at n <= 129 and is covered by the one-term slack of using n = rows
    where n - 1 additions involve two non-zero operands.  The float64 reference's own error (u64 = 2^-53) is 2^-29 of that."""
    for rows, nR, H, density in ((10, 4, 3, 0.5), (30, 20, 16, 0.3), (65, 8, 5, 0.7), (128, 12, 9, 1.0)):
        dyn, bits, W, b = M.random_case(5, rows, nR, H, density, rows + 7, spiky=False)
        got = M.encode(bits, W, b, rows, nR)
        want, mag = M.encode64(dyn, W, b)
        assert got.dtype == np.float32 and got.shape == (5, H, nR)
        assert (np.abs(got.astype(np.float64) - want) <= rows * M.U32 * mag).all()
        # the same bound through the weights alone, as the GPU tests state it: rows * 2^-24 * (sum_r |W[h, r]| + |b[h]|)
        wide = rows * M.U32 * (np.abs(W.astype(np.float64)).sum(1) + np.abs(b.astype(np.float64)))
        assert (np.abs(got.astype(np.float64) - want) <= wide[None, :, None]).all()
    # an all-zero shadow gives exactly the bias; without a bias exactly +0
    z = np.zeros((2, 4), np.int64)
    W = np.random.RandomState(1).randn(3, 10).astype(np.float32)
    b = np.array([1.5, -2.0, 1e-30], np.float32)
    assert np.array_equal(M.encode(z, W, b, 10, 4), np.broadcast_to(b[None, :, None], (2, 3, 4)))
    assert not M.encode(z, W, None, 10, 4).any()
    # the order matters on the spiky row: this is what makes a reordered device sum visible
    dyn, bits, W, b = M.random_case(4, 30, 8, 6, 1.0, 3)
    seq = M.encode(bits, W, None, 30, 8)
    rev = M.encode(M.pack_bits(dyn[:, ::-1, :]), W[:, ::-1], None, 30, 8)
    assert not np.array_equal(seq[:, 3], rev[:, 3])
