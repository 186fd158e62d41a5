"""The model of the pointer network's static-rows form (tapenv.h: tap_pointer_scores_static), what
tests/test_pointer_static_cpu.py and tests/test_pointer_static_gpu.py share.  tests/pointer_model.py has the reference's
form and the folded contract on a given ``proj``; here static_hidden is what it is in the actor, a 1x1 convolution of the
S rows ``xs`` of ``static`` that the static encoder sees -- static_hidden = Es . xs + bs --, and the contract's static term
is P = g + G . xs with G = Ws . Es (3 Hd, S), g = Ws . bs (3 Hd,).

    make_case           pointer_model.make_case plus a static encoder (Es xavier, bs small) and xs (integers 1 .. 8 as floats,
                        a block's sides); static_hidden is the float64 convolution
    fold                -> G, g, M, k, q in float64
    static_term         P (B, 3 Hd, nR) from xs, G, g in a given dtype (numpy)
    folded_torch        the contract in torch, differentiable: pointer_model.folded_torch on P
    reference_form_torch  the reference's own ops with the static encoder's convolution in front, in a given dtype: its
                        float32 run against its float64 run is e_ref"""
import numpy as np
import torch

import pointer_model as M


def make_case(B, rows, nR, He, Hd, S, density, seed):
    X = M.make_case(B, rows, nR, He, Hd, density, seed)
    rng = np.random.RandomState(seed + 7919)
    X["S"] = S
    X["Es"] = M._xavier(rng, (He, S))
    X["bs"] = (0.1 * rng.randn(He)).astype(np.float32)
    X["xs"] = rng.randint(1, 9, size=(B, S, nR)).astype(np.float32)
    X["static_hidden"] = static_hidden(X, np.float64)
    return X


def static_hidden(X, dtype=np.float64):
    c = lambda a: np.asarray(a, dtype)
    return np.einsum('hs,bsc->bhc', c(X["Es"]), c(X["xs"])) + c(X["bs"])[None, :, None]


def fold(X, dtype=np.float64):
    """-> G (3 Hd, S), g (3 Hd,), M (3 Hd, rows), k (3 Hd,), q (B, Hd)"""
    c = lambda a: np.asarray(a, dtype)
    He = X["He"]
    Wa, Wp = c(X["Wa"]), c(X["Wp"])
    Ws = np.concatenate((Wa[:, :He], Wp[:, :He], Wp[:, 2 * He:3 * He]), 0)
    _, Mf, k, q = M.fold(X, dtype)
    return Ws @ c(X["Es"]), Ws @ c(X["bs"]), Mf, k, q


def static_term(xs, G, g, dtype=np.float64):
    """P[b, x, c] = g[x] + sum_i G[x, i] xs[b, i, c], i ascending, every operation in ``dtype``"""
    xs, G, g = (np.asarray(a, dtype) for a in (xs, G, g))
    P = np.broadcast_to(g[None, :, None], (xs.shape[0], G.shape[0], xs.shape[2])).astype(dtype)
    for i in range(G.shape[1]):
        P = P + G[None, :, i, None] * xs[:, None, i, :]
    assert P.dtype == dtype
    return P


def folded_torch(xs, G, g, dynf, Mf, k, q, va, vp):
    """the static-rows contract in torch, differentiable in everything but xs -> logits, attn, t"""
    P = g[None, :, None] + torch.einsum('xs,bsc->bxc', G, xs)
    return M.folded_torch(P, dynf, Mf, k, q, va, vp)


def reference_form_torch(X, dtype):
    """pointer_model.reference_form_torch with static_hidden = conv1d(xs, Es, bs) computed in ``dtype`` first"""
    c = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    Y = dict(X)
    Y["static_hidden"] = torch.nn.functional.conv1d(c(X["xs"]), c(X["Es"])[:, :, None], c(X["bs"])).numpy()
    return M.reference_form_torch(Y, dtype)
