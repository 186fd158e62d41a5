"""The model of the state critic on the bit shadow (tapenv.h: tap_critic_value), the tests' oracle: the reference's form
(trainer.py:18-94 after the GRU step: a Conv1d over the fp32 dynamic, then per process block a concatenation, a bmm, a
softmax and a context bmm) and the folded form the kernel computes, each in numpy and in torch, in float64 or float32.

Notation: H the hidden size, S the static rows, n the process blocks; Es, bs / Ed, bd the static / dynamic encoder's
conv.weight[:, :, 0] and conv.bias; W = attention.W[0] (H, 3 H), columns [Was | Wad | Waq]; v = attention.v[0, 0];
F1, f1 = fc.0; w2 (H,), b2 (1,) = fc.2.  Folded: G = [Was Es; Waq Es; F1 Es] (3 H, S), g = [Was bs + Wad bd; Waq bs;
F1 bs + f1], M = Wad Ed (H, rows), q0 = rnn_out Waq^T, and per env
    U = g[:H] + sum of M[:, r] over the set rows r (ascending) + G[:H] x;  per block: s = v . tanh(U + q), p = softmax(s),
    xbar = x p, q = g[H:2H] + G[H:2H] xbar;  z = g[2H:] + G[2H:] xbar;  value = b2 + w2 . relu(z)."""
import numpy as np
import torch

from pointer_model import U32, _xavier, garbage, pack_bits, planes_of, tolerance, unpack_bits   # noqa: F401

NAMES = ("value", "z", "p", "xbar")


def make_case(B, rows, nR, H, S, n, density, seed):
    """the reference form's inputs, float32 values: xavier-scaled weights (v four times that: the softmax is not flat),
    block sides 1..5 as the static input, a 0/1 dynamic at ``density`` and rnn_out = tanh of a normal"""
    rng = np.random.RandomState(seed)
    return dict(H=H, S=S, n=n, rows=rows, nR=nR,
                x=rng.randint(1, 6, size=(B, S, nR)).astype(np.float32),
                dyn=rng.rand(B, rows, nR) < density,
                Es=_xavier(rng, (H, S)), bs=(0.1 * rng.randn(H)).astype(np.float32),
                Ed=_xavier(rng, (H, rows)), bd=(0.1 * rng.randn(H)).astype(np.float32),
                W=_xavier(rng, (H, 3 * H)), v=4 * _xavier(rng, (1, H))[0],
                F1=_xavier(rng, (H, H)), f1=(0.1 * rng.randn(H)).astype(np.float32),
                w2=_xavier(rng, (1, H))[0], b2=(0.1 * rng.randn(1)).astype(np.float32),
                rnn_out=np.tanh(rng.randn(B, H)).astype(np.float32))


def _softmax(s):
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def reference_form(X, dtype=np.float64):
    """trainer.py:29-42 and 76-94 restated in numpy -> value (B,), z (B, H) = fc.0's output, p (B, n, nR), xbar (B, n, S)"""
    c = lambda a: np.asarray(a, dtype)
    x, r = c(X["x"]), c(X["rnn_out"])
    sh = np.einsum('hs,bsc->bhc', c(X["Es"]), x) + c(X["bs"])[None, :, None]
    dh = np.einsum('hr,brc->bhc', c(X["Ed"]), c(X["dyn"])) + c(X["bd"])[None, :, None]
    ps, xs = [], []
    for _ in range(X["n"]):
        hidden = np.concatenate((sh, dh, np.repeat(r[:, :, None], sh.shape[2], 2)), 1)
        p = _softmax(np.einsum('j,bjc->bc', c(X["v"]), np.tanh(np.einsum('jx,bxc->bjc', c(X["W"]), hidden))))
        r = np.einsum('bc,bhc->bh', p, sh)
        ps.append(p)
        xs.append(np.einsum('bc,bsc->bs', p, x))
    z = r @ c(X["F1"]).T + c(X["f1"])
    value = np.maximum(z, 0) @ c(X["w2"]) + c(X["b2"])[0]
    assert value.dtype == dtype
    return value, z, np.stack(ps, 1), np.stack(xs, 1)


def fold(X, dtype=np.float64):
    """-> G (3 H, S), g (3 H,), M (H, rows), q0 (B, H)"""
    c = lambda a: np.asarray(a, dtype)
    H = X["H"]
    W, Es, bs, Ed, bd, F1 = c(X["W"]), c(X["Es"]), c(X["bs"]), c(X["Ed"]), c(X["bd"]), c(X["F1"])
    Was, Wad, Waq = W[:, :H], W[:, H:2 * H], W[:, 2 * H:]
    G = np.concatenate((Was @ Es, Waq @ Es, F1 @ Es), 0)
    g = np.concatenate((Was @ bs + Wad @ bd, Waq @ bs, F1 @ bs + c(X["f1"])), 0)
    return G, g, Wad @ Ed, c(X["rnn_out"]) @ Waq.T


def folded(x, dyn, G, g, M, q0, v, w2, b2, n, dtype=np.float64):
    """the contract on the 0/1 ``dyn`` (B, rows, nR) -> value, z, p, xbar.  The sum over the set rows is sequential in
    ascending row order, starting from g, and G . x is added last, as the contract orders it"""
    c = lambda a: np.asarray(a, dtype)
    x, G, g, M, q, v, w2, b2 = c(x), c(G), c(g), c(M), c(q0), c(v), c(w2), c(b2)
    B, S, nR = x.shape
    H = M.shape[0]
    U = np.broadcast_to(g[None, :H, None], (B, H, nR)).astype(dtype)
    zero = dtype(0)
    for r in range(dyn.shape[1]):
        U = U + np.where(dyn[:, r, :][:, None, :], M[:, r][None, :, None], zero)
    for i in range(S):
        U = U + G[None, :H, i, None] * x[:, None, i, :]
    q = np.broadcast_to(q, (B, H))
    ps, xs = [], []
    for _ in range(n):
        p = _softmax(np.einsum('j,bjc->bc', v, np.tanh(U + q[:, :, None])))
        xbar = np.einsum('bc,bsc->bs', p, x)
        q = g[None, H:2 * H] + xbar @ G[H:2 * H].T
        ps.append(p)
        xs.append(xbar)
    z = g[None, 2 * H:] + xs[-1] @ G[2 * H:].T
    value = np.maximum(z, 0) @ w2 + b2.reshape(-1)[0]
    assert value.dtype == dtype
    return value, z, np.stack(ps, 1), np.stack(xs, 1)


# ---- the same two forms in torch (float32 for the reference's own error, float64 autograd for the gradients) ----------
def reference_form_torch(X, dtype):
    """the reference's lines with its own ops (conv1d, cat, expand, bmm, softmax, Linear) on the CPU -> value, z, p, xbar"""
    c = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    H = X["H"]
    x, r = c(X["x"]), c(X["rnn_out"])
    B = x.shape[0]
    F = torch.nn.functional
    sh = F.conv1d(x, c(X["Es"])[:, :, None], c(X["bs"]))
    dh = F.conv1d(c(X["dyn"].astype(np.float32)), c(X["Ed"])[:, :, None], c(X["bd"]))
    v, W = c(X["v"]).view(1, 1, H).expand(B, 1, H), c(X["W"]).unsqueeze(0).expand(B, H, -1)
    ps, xs = [], []
    for _ in range(X["n"]):
        hidden = torch.cat((sh, dh, r.unsqueeze(2).expand_as(sh)), 1)
        prob = torch.softmax(torch.bmm(v, torch.tanh(torch.bmm(W, hidden))), dim=2)
        r = prob.bmm(sh.permute(0, 2, 1)).squeeze(1)
        ps.append(prob.squeeze(1))
        xs.append(prob.bmm(x.permute(0, 2, 1)).squeeze(1))
    z = F.linear(r, c(X["F1"]), c(X["f1"]))
    value = F.linear(torch.relu(z), c(X["w2"]).view(1, H), c(X["b2"])).squeeze(1)
    return value, z, torch.stack(ps, 1), torch.stack(xs, 1)


def folded_torch(x, dynf, G, g, M, q0, v, w2, b2, n):
    """the contract in torch on a floating 0/1 ``dynf``, differentiable -> value, z, p, xbar"""
    H = M.shape[0]
    B = x.shape[0]
    U = g[None, :H, None] + torch.einsum('jr,brc->bjc', M, dynf) + torch.einsum('js,bsc->bjc', G[:H], x)
    q = q0.expand(B, H)
    ps, xs = [], []
    for _ in range(n):
        p = torch.softmax(torch.einsum('j,bjc->bc', v, torch.tanh(U + q[:, :, None])), dim=1)
        xbar = torch.einsum('bc,bsc->bs', p, x)
        q = g[None, H:2 * H] + xbar.matmul(G[H:2 * H].t())
        ps.append(p)
        xs.append(xbar)
    z = g[None, 2 * H:] + xs[-1].matmul(G[2 * H:].t())
    value = torch.relu(z).matmul(w2) + b2.reshape(-1)[0]
    return value, z, torch.stack(ps, 1), torch.stack(xs, 1)
