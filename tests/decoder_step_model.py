"""The model of the decoder step (tapenv.h: tap_decoder_step), the tests' oracle: the reference's form (model.py:347-354
and 108-115: two 1x1 convolutions, a concatenation, nn.GRU for one step, then the decoder's columns of the attention's W)
and the folded form the kernel computes, in numpy and in torch, in float64 or float32.

Per env: xs (Ks) the chosen block's sides, xd (Kd) the container feature, h (Hd) the previous hidden state, K = Ks + Kd.
    gi = P . [xs ; xd] + c                     P (3 Hd, K), c (3 Hd): gate order r, z, n as nn.GRU lays weight_ih out
    gh = W_hh . h + b_hh
    r  = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z);  n = tanh(gi_n + r gh_n)
    h' = (1 - z) n + z h
    q  = Wq . h'                               Wq = encoder_attn.W[0][:, 2 He:]
P, c fold the decoder's encoders (Ws, bs of os rows; Wd, bd of od rows) into W_ih, b_ih:
    'cat' (os + od = Hd):  P = [W_ih[:, :os] Ws | W_ih[:, os:] Wd],  c = W_ih cat(bs, bd) + b_ih
    'sum' (os = od = Hd):  P = [W_ih Ws | W_ih Wd],                  c = W_ih (bs + bd) + b_ih
a missing encoder has width 0; ``identity`` m: the dynamic half arrives encoded (m rows) and Wd is the m x m identity.

The order of every sum, fixed by the shape (``step`` follows it term by term):
  * gi_g[j]: starts from c[g Hd + j]; the K input terms are added in ascending order, the Ks static columns first;
  * gh_g[j]: starts from b_hh[g Hd + j]; the Hd hidden terms are added in ascending order (a null h: gh = b_hh exactly);
  * q[j]: starts from 0; the Hd terms of h' are added in ascending order;
  * r gh_n, (1 - z) n and z h are rounded before they are added.
On the device every addition of a term is one fmaf (the product is not rounded); numpy rounds the product too, which is
why the float32 run of ``step`` is a restatement of the order and not bit-for-bit the kernel."""
import numpy as np
import torch

from pointer_model import _xavier, tolerance   # noqa: F401  (the project's tolerance rule)


def make_case(B, Ks, Kd, Hd, seed, combine='cat', identity=0):
    """the reference form's inputs, float32 values: xavier-uniform matrices, small normal biases, x the small
    non-negative integers a stepper produces (0 .. 50; an encoded ``identity`` half is unit normal), h = tanh of a normal"""
    rng = np.random.RandomState(seed)
    if combine == 'cat':
        os_ = 0 if Ks == 0 else Hd if Kd == 0 else (Hd - identity if identity else Hd // 2)
        od = Hd - os_
    else:
        os_ = od = Hd
    assert not identity or identity == od == Kd
    bias = lambda n: (0.1 * rng.randn(n)).astype(np.float32)
    X = dict(B=B, Ks=Ks, Kd=Kd, Hd=Hd, combine=combine, identity=identity, os=os_ if Ks else 0, od=od if Kd else 0,
             Ws=_xavier(rng, (os_, max(Ks, 1)))[:, :Ks], bs=bias(os_),
             Wd=np.eye(identity, dtype=np.float32) if identity else _xavier(rng, (od, max(Kd, 1)))[:, :Kd],
             bd=np.zeros(identity, np.float32) if identity else bias(od),
             W_ih=_xavier(rng, (3 * Hd, Hd)), W_hh=_xavier(rng, (3 * Hd, Hd)), b_ih=bias(3 * Hd), b_hh=bias(3 * Hd),
             Wq=np.ascontiguousarray(_xavier(rng, (Hd, 3 * Hd))[:, 2 * Hd:]),
             xs=rng.randint(0, 51, (B, Ks)).astype(np.float32),
             xd=rng.randn(B, Kd).astype(np.float32) if identity else rng.randint(0, 51, (B, Kd)).astype(np.float32),
             h=np.tanh(rng.randn(B, Hd)).astype(np.float32))
    return X


def fold(X, dtype=np.float64):
    """-> P (3 Hd, K), c (3 Hd,)"""
    f = lambda a: np.asarray(a, dtype)
    W_ih, Ws, Wd, bs, bd = f(X["W_ih"]), f(X["Ws"]), f(X["Wd"]), f(X["bs"]), f(X["bd"])
    Ks, Kd, os_ = X["Ks"], X["Kd"], X["os"]
    if X["combine"] == 'cat':
        halves = ([W_ih[:, :os_] @ Ws] if Ks else []) + ([W_ih[:, os_:] @ Wd] if Kd else [])
        b = np.concatenate(([bs] if Ks else []) + ([bd] if Kd else []))
    else:
        halves = ([W_ih @ Ws] if Ks else []) + ([W_ih @ Wd] if Kd else [])
        b = (bs if Ks else 0) + (bd if Kd else 0)
    return np.concatenate(halves, axis=1), W_ih @ b + f(X["b_ih"])


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def step(xs, xd, h, P, c, w_hh, b_hh, wq, dtype=np.float64):
    """the contract in numpy, every sum in the documented order -> h' (B, Hd), q (B, Hd), gates (B, 4, Hd) = r, z, n, gh_n.
    ``h`` None is the zero state: gh = b_hh exactly"""
    f = lambda a: np.asarray(a, dtype)
    x = np.concatenate((f(xs), f(xd)), axis=1)
    P, c, w_hh, b_hh, wq = f(P), f(c), f(w_hh), f(b_hh), f(wq)
    B, Hd = x.shape[0], wq.shape[0]
    gi = np.broadcast_to(c, (B, 3 * Hd)).astype(dtype)
    for k in range(x.shape[1]):
        gi = gi + x[:, k:k + 1] * P[:, k][None, :]
    gh = np.broadcast_to(b_hh, (B, 3 * Hd)).astype(dtype)
    hp = np.zeros((B, Hd), dtype) if h is None else f(h)
    if h is not None:
        for k in range(Hd):
            gh = gh + hp[:, k:k + 1] * w_hh[:, k][None, :]
    r = _sigmoid(gi[:, :Hd] + gh[:, :Hd])
    z = _sigmoid(gi[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
    n = np.tanh(gi[:, 2 * Hd:] + r * gh[:, 2 * Hd:])
    hn = (1 - z) * n + z * hp
    q = np.zeros((B, Hd), dtype)
    for k in range(Hd):
        q = q + hn[:, k:k + 1] * wq[:, k][None, :]
    gates = np.stack((r, z, n, gh[:, 2 * Hd:]), axis=1)
    assert hn.dtype == dtype and q.dtype == dtype and gates.dtype == dtype
    return hn, q, gates


def step_torch(xs, xd, h, P, c, w_hh, b_hh, wq):
    """the contract in torch, differentiable (the sums are matmuls) -> h', q, gates"""
    x = torch.cat((xs, xd), dim=1)
    Hd = wq.shape[0]
    gi = x.matmul(P.t()) + c
    gh = b_hh.expand(x.shape[0], -1) if h is None else h.matmul(w_hh.t()) + b_hh
    r = torch.sigmoid(gi[:, :Hd] + gh[:, :Hd])
    z = torch.sigmoid(gi[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
    n = torch.tanh(gi[:, 2 * Hd:] + r * gh[:, 2 * Hd:])
    hn = (1 - z) * n + (0 if h is None else z * h)
    return hn, hn.matmul(wq.t()), torch.stack((r, z, n, gh[:, 2 * Hd:]), dim=1)


def reference_modules(X, dtype):
    """the reference's own modules holding the case's weights: the two nn.Conv1d encoders (None for a missing or an
    identity half) and the nn.GRU (one layer, batch_first)"""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)

    def conv(W, b):
        m = torch.nn.Conv1d(W.shape[1], W.shape[0], 1).to(dtype)
        with torch.no_grad():
            m.weight.copy_(t(W)[:, :, None])
            m.bias.copy_(t(b))
        return m
    enc_s = conv(X["Ws"], X["bs"]) if X["Ks"] else None
    enc_d = conv(X["Wd"], X["bd"]) if X["Kd"] and not X["identity"] else None
    gru = torch.nn.GRU(X["Hd"], X["Hd"], 1, batch_first=True).to(dtype)
    with torch.no_grad():
        for name in ("W_ih", "W_hh", "b_ih", "b_hh"):
            getattr(gru, {"W": "weight", "b": "bias"}[name[0]] + name[1:] + "_l0").copy_(t(X[name]))
    return enc_s, enc_d, gru


def reference_form_torch(X, dtype, with_h=True):
    """model.py:347-354 and 108-115 with the reference's own ops on the CPU: nn.Conv1d encoders -> cat / sum -> nn.GRU, one
    step from h (or from None) -> Wq.  -> h' (B, Hd), q (B, Hd)"""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    enc_s, enc_d, gru = reference_modules(X, dtype)
    halves = []
    if X["Ks"]:
        halves.append(enc_s(t(X["xs"])[:, :, None]))
    if X["Kd"]:
        halves.append(t(X["xd"])[:, :, None] if X["identity"] else enc_d(t(X["xd"])[:, :, None]))
    decoder_hidden = torch.cat(halves, dim=1) if X["combine"] == 'cat' else sum(halves)
    rnn_out, last_hh = gru(decoder_hidden.transpose(2, 1), t(X["h"])[None] if with_h else None)
    assert torch.equal(rnn_out.squeeze(1), last_hh[0])                     # one layer, one step
    return last_hh[0], rnn_out.squeeze(1).matmul(t(X["Wq"]).t())
