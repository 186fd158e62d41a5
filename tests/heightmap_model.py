"""The model of the 3D decoder step (tapenv.h: tap_decoder_step_hm), the tests' oracle: the reference's HeightmapEncoder
(model.py:21-35) restated on the cells it reads, term by term in the documented order, then decoder_step_model.step with
xd = enc; in numpy (float64 or float32) and, for the gradients and e_ref, in torch with the reference's own ops.

Per env, hm (C, W, L), nw = ceil(W / 4), nl = ceil(L / 4), Np = nw nl, p = i nl + j, C1 = m / 4, C2 = m / 2:
    a1[p, o] = leaky(b1[o] + sum_c  w1[o, c]  hm[c, 4i, 4j])          c ascending
    a2[p, o] = leaky(b2[o] + sum_c1 w2[o, c1] a1[p, c1])             c1 ascending
    enc[o]   = b3[o] + sum_t w3[o, t] a2flat[t]                      t = c2 Np + p ascending (conv3.weight's memory order)
    leaky(x) = x > 0 ? x : 0.01 x
On the device every addition of a term is one fmaf and the slope is 0.01f; numpy rounds the product too, so the float32
run is a restatement of the order and not bit for bit the kernel."""
import numpy as np
import torch
from torch.nn import functional as F

import decoder_step_model as DM
from pointer_model import tolerance   # noqa: F401  (the project's tolerance rule)


def _xavier_conv(rng, shape):
    """torch's xavier_uniform_ on a convolution weight (out, in, kh, kw)"""
    rf = int(np.prod(shape[2:]))
    a = np.sqrt(6.0 / ((shape[0] + shape[1]) * rf))
    return rng.uniform(-a, a, size=shape).astype(np.float32)


def make_encoder(rng, C, m, W, L):
    """-> [w1, b1, w2, b2, w3, b3] float32 in the modules' own shapes"""
    nw, nl = (W + 3) // 4, (L + 3) // 4
    bias = lambda n: (0.1 * rng.randn(n)).astype(np.float32)                          # noqa: E731
    return [_xavier_conv(rng, (m // 4, C, 1, 1)), bias(m // 4), _xavier_conv(rng, (m // 2, m // 4, 1, 1)), bias(m // 2),
            _xavier_conv(rng, (m, m // 2, nw, nl)), bias(m)]


def make_case(B, Ks, C, W, L, m, Hd, seed, combine='cat'):
    """the reference form's inputs, float32 values: a Conv1d static encoder (Ws, bs) of Hd - m rows ('cat') or Hd rows
    ('sum'; m = Hd), the height-map encoder, the GRU, Wq; hm integers in [-50, 50], xs in 0 .. 50, h = tanh of a normal"""
    rng = np.random.RandomState(seed)
    os_ = (Hd - m if combine == 'cat' else Hd) if Ks else 0
    assert (os_ + m == Hd) if combine == 'cat' else m == Hd
    bias = lambda n: (0.1 * rng.randn(n)).astype(np.float32)                          # noqa: E731
    return dict(B=B, Ks=Ks, C=C, W=W, L=L, m=m, Hd=Hd, combine=combine, os=os_,
                Ws=DM._xavier(rng, (os_, max(Ks, 1)))[:, :Ks], bs=bias(os_), enc=make_encoder(rng, C, m, W, L),
                W_ih=DM._xavier(rng, (3 * Hd, Hd)), W_hh=DM._xavier(rng, (3 * Hd, Hd)), b_ih=bias(3 * Hd), b_hh=bias(3 * Hd),
                Wq=np.ascontiguousarray(DM._xavier(rng, (Hd, 3 * Hd))[:, 2 * Hd:]),
                xs=rng.randint(0, 51, (B, Ks)).astype(np.float32),
                hm=rng.randint(-50, 51, (B, C, W, L)).astype(np.float32),
                h=np.tanh(rng.randn(B, Hd)).astype(np.float32))


def fold(X, dtype=np.float64):
    """-> P (3 Hd, Ks + m), c (3 Hd,): the static encoder folded, m identity columns and no bias for the dynamic half"""
    f = lambda a: np.asarray(a, dtype)                                                # noqa: E731
    W_ih, Ws, bs, os_ = f(X["W_ih"]), f(X["Ws"]), f(X["bs"]), X["os"]
    if X["combine"] == 'cat':
        P = np.concatenate(([W_ih[:, :os_] @ Ws] if X["Ks"] else []) + [W_ih[:, os_:]], axis=1)
        c = (W_ih[:, :os_] @ bs if X["Ks"] else 0) + f(X["b_ih"])
    else:
        P = np.concatenate(([W_ih @ Ws] if X["Ks"] else []) + [W_ih], axis=1)
        c = (W_ih @ bs if X["Ks"] else 0) + f(X["b_ih"])
    return P, c


def _leaky(x):
    return np.where(x > 0, x, x.dtype.type(0.01) * x)


def encode(hm, enc_w, dtype=np.float64):
    """the encoder stage in numpy, every sum in the documented order -> enc (B, m), z1 (B, Np, C1), z2 (B, Np, C2) (the two
    hidden layers before their leaky-ReLU)"""
    f = lambda a: np.asarray(a, dtype)                                                # noqa: E731
    hm = f(hm)
    w1, b1, w2, b2, w3, b3 = (f(a) for a in enc_w)
    B, C = hm.shape[:2]
    cells = hm[:, :, ::4, ::4]
    nw, nl = cells.shape[2:]
    assert (nw, nl) == ((hm.shape[2] + 3) // 4, (hm.shape[3] + 3) // 4) == tuple(w3.shape[2:])
    Np, C1, C2, m = nw * nl, w1.shape[0], w2.shape[0], w3.shape[0]
    cells = cells.reshape(B, C, Np)                                  # p = i nl + j
    w1, w2, w3 = w1.reshape(C1, C), w2.reshape(C2, C1), w3.reshape(m, C2 * Np)
    z1 = np.broadcast_to(b1, (B, Np, C1)).astype(dtype)
    for c in range(C):
        z1 = z1 + cells[:, c, :, None] * w1[None, None, :, c]
    a1 = _leaky(z1)
    z2 = np.broadcast_to(b2, (B, Np, C2)).astype(dtype)
    for c1 in range(C1):
        z2 = z2 + a1[:, :, c1:c1 + 1] * w2[None, None, :, c1]
    a2 = _leaky(z2).transpose(0, 2, 1).reshape(B, C2 * Np)            # t = c2 Np + p
    enc = np.broadcast_to(b3, (B, m)).astype(dtype)
    for t in range(C2 * Np):
        enc = enc + a2[:, t:t + 1] * w3[None, :, t]
    assert enc.dtype == dtype
    return enc, z1, z2


def step(xs, hm, h, enc_w, P, c, w_hh, b_hh, wq, dtype=np.float64):
    """the contract in numpy -> h' (B, Hd), q (B, Hd), gates (B, 4, Hd), enc (B, m)"""
    enc = encode(hm, enc_w, dtype)[0]
    return DM.step(xs, enc, h, P, c, w_hh, b_hh, wq, dtype) + (enc,)


def encode_torch(hm, enc_w):
    """model.py:30-35 with the reference's own ops, differentiable -> (B, m)"""
    w1, b1, w2, b2, w3, b3 = enc_w
    out = F.leaky_relu(F.conv2d(hm, w1, b1, stride=2))
    out = F.leaky_relu(F.conv2d(out, w2, b2, stride=2))
    return F.conv2d(out, w3, b3).squeeze(-1).squeeze(-1)


def step_torch(xs, hm, h, enc_w, P, c, w_hh, b_hh, wq):
    """the reference's encoder, then the folded step in torch, differentiable -> h', q, gates, enc"""
    enc = encode_torch(hm, enc_w)
    return DM.step_torch(xs, enc, h, P, c, w_hh, b_hh, wq) + (enc,)


def reference_form_torch(X, dtype, with_h=True):
    """model.py:347-354 and 108-115 with the reference's own ops on the CPU: nn.Conv1d static encoder and the HeightmapEncoder's
    three convolutions -> cat / sum -> nn.GRU, one step -> Wq.  -> h' (B, Hd), q (B, Hd), enc (B, m)"""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)                           # noqa: E731
    enc = encode_torch(t(X["hm"]), [t(a) for a in X["enc"]])
    halves = []
    if X["Ks"]:
        halves.append(F.conv1d(t(X["xs"])[:, :, None], t(X["Ws"])[:, :, None], t(X["bs"])))
    halves.append(enc[:, :, None])
    decoder_hidden = torch.cat(halves, dim=1) if X["combine"] == 'cat' else sum(halves)
    gru = torch.nn.GRU(X["Hd"], X["Hd"], 1, batch_first=True).to(dtype)
    with torch.no_grad():
        for name in ("W_ih", "W_hh", "b_ih", "b_hh"):
            getattr(gru, {"W": "weight", "b": "bias"}[name[0]] + name[1:] + "_l0").copy_(t(X[name]))
    rnn_out, last_hh = gru(decoder_hidden.transpose(2, 1), t(X["h"])[None] if with_h else None)
    return last_hh[0], rnn_out.squeeze(1).matmul(t(X["Wq"]).t()), enc
