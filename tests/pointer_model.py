"""The model of the pointer network on the bit shadow (tapenv.h: tap_pointer_scores), the tests' oracle: the reference's
form (model.py:38-138 after the GRU step: two concatenations, two W, a softmax, a context) and the folded form the
kernel computes, each in numpy and in torch, in float64 or float32.

Notation: He / Hd the encoder / decoder hidden sizes; Wa = encoder_attn.W[0] (Hd, 2 He + Hd), columns [static | dynamic
| decoder]; Wp = W[0] (Hd, 4 He), columns [static | dynamic | ctx static | ctx dynamic]; va / vp the two v; We, be the
dynamic encoder's conv.weight[:, :, 0] and conv.bias.  Folded: Ws = [Wa[:, :He]; Wp[:, :He]; Wp[:, 2He:3He]], Wd =
[Wa[:, He:2He]; Wp[:, He:2He]; Wp[:, 3He:4He]], proj = Ws . static_hidden, M = Wd . We, k = Wd . be, q = rnn_out .
Wa[:, 2He:]^T, and per env and column
    U = proj + (k + sum of M[:, r] over the set rows r, ascending);  s = va . tanh(U[:Hd] + q);  attn = softmax(s);
    t = U[2Hd:] . attn;  logits = vp . tanh(U[Hd:2Hd] + t)."""
import numpy as np
import torch

from dyn_encoder_model import U32, garbage, pack_bits, planes_of, unpack_bits   # noqa: F401  (the shadow's layout)


def _xavier(rng, shape):
    """Xavier-uniform on the last two axes, as the reference initialises every parameter with more than one axis"""
    a = np.sqrt(6.0 / (shape[-1] + shape[-2]))
    return rng.uniform(-a, a, size=shape).astype(np.float32)


def make_case(B, rows, nR, He, Hd, density, seed):
    """the reference form's inputs, float32 values: xavier-scaled weights, a unit-normal static_hidden, a 0/1 dynamic at
    ``density`` and rnn_out = tanh of a normal (a GRU's output lies in (-1, 1))"""
    rng = np.random.RandomState(seed)
    return dict(He=He, Hd=Hd, rows=rows, nR=nR,
                static_hidden=rng.randn(B, He, nR).astype(np.float32),
                dyn=rng.rand(B, rows, nR) < density,
                We=_xavier(rng, (He, rows)), be=(0.1 * rng.randn(He)).astype(np.float32),
                Wa=_xavier(rng, (Hd, 2 * He + Hd)), va=_xavier(rng, (1, Hd))[0],
                Wp=_xavier(rng, (Hd, 4 * He)), vp=_xavier(rng, (1, Hd))[0],
                rnn_out=np.tanh(rng.randn(B, Hd)).astype(np.float32))


def _softmax(s):
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def reference_form(X, dtype=np.float64):
    """model.py:55-74 and 119-136 restated in numpy -> logits (B, nR), attn (B, nR), and t (B, Hd) = what W's context
    columns give (the one intermediate the folded form names that the reference's single product hides)"""
    c = lambda a: np.asarray(a, dtype)
    He = X["He"]
    sh, Wa, va, Wp, vp, r = c(X["static_hidden"]), c(X["Wa"]), c(X["va"]), c(X["Wp"]), c(X["vp"]), c(X["rnn_out"])
    dh = np.einsum('hr,brc->bhc', c(X["We"]), c(X["dyn"])) + c(X["be"])[None, :, None]
    enc = np.concatenate((sh, dh), 1)                                            # (B, 2 He, nR)
    hidden = np.concatenate((enc, np.repeat(r[:, :, None], sh.shape[2], 2)), 1)
    attn = _softmax(np.einsum('j,bjc->bc', va, np.tanh(np.einsum('jx,bxc->bjc', Wa, hidden))))
    context = np.einsum('bc,bxc->bx', attn, enc)                                 # (B, 2 He)
    energy = np.concatenate((enc, np.repeat(context[:, :, None], sh.shape[2], 2)), 1)
    logits = np.einsum('j,bjc->bc', vp, np.tanh(np.einsum('jx,bxc->bjc', Wp, energy)))
    t = np.einsum('jx,bx->bj', Wp[:, 2 * He:], context)
    assert logits.dtype == dtype
    return logits, attn, t


def fold(X, dtype=np.float64):
    """-> proj (B, 3 Hd, nR) in the contract's natural order, M (3 Hd, rows), k (3 Hd,), q (B, Hd)"""
    c = lambda a: np.asarray(a, dtype)
    He = X["He"]
    Wa, Wp = c(X["Wa"]), c(X["Wp"])
    Ws = np.concatenate((Wa[:, :He], Wp[:, :He], Wp[:, 2 * He:3 * He]), 0)
    Wd = np.concatenate((Wa[:, He:2 * He], Wp[:, He:2 * He], Wp[:, 3 * He:4 * He]), 0)
    proj = np.einsum('xh,bhc->bxc', Ws, c(X["static_hidden"]), optimize=True)
    return proj, Wd @ c(X["We"]), Wd @ c(X["be"]), c(X["rnn_out"]) @ Wa[:, 2 * He:].T


def to_layout(proj):
    """(B, 3 Hd, nR) -> the kernel's (B, 3, nR, Hd): segment-major, hidden fastest"""
    B, H3, nR = proj.shape
    return np.ascontiguousarray(proj.reshape(B, 3, H3 // 3, nR).transpose(0, 1, 3, 2))


def from_layout(p4):
    B, _, nR, Hd = p4.shape
    return np.ascontiguousarray(p4.transpose(0, 1, 3, 2)).reshape(B, 3 * Hd, nR)


def folded(proj, dyn, M, k, q, va, vp, dtype=np.float64):
    """the contract on (B, 3 Hd, nR) proj and the 0/1 ``dyn`` (B, rows, nR) -> logits, attn, t.  The sum over the set
    rows is sequential in ascending row order, starting from k, and proj is added last, as the contract orders it"""
    c = lambda a: np.asarray(a, dtype)
    proj, M, k, q, va, vp = c(proj), c(M), c(k), c(q), c(va), c(vp)
    Hd = q.shape[1]
    acc = np.broadcast_to(k[None, :, None], proj.shape).astype(dtype)
    zero = dtype(0)
    for r in range(dyn.shape[1]):
        acc = acc + np.where(dyn[:, r, :][:, None, :], M[:, r][None, :, None], zero)
    U = proj + acc
    attn = _softmax(np.einsum('j,bjc->bc', va, np.tanh(U[:, :Hd] + q[:, :, None])))
    t = np.einsum('bc,bjc->bj', attn, U[:, 2 * Hd:])
    logits = np.einsum('j,bjc->bc', vp, np.tanh(U[:, Hd:2 * Hd] + t[:, :, None]))
    assert logits.dtype == dtype
    return logits, attn, t


# ---- the same two forms in torch (float32 for the reference's own error, float64 autograd for the gradients) ----------
def reference_form_torch(X, dtype):
    """the reference's lines with its own ops (cat, repeat, expand, bmm, softmax) on the CPU -> logits, attn, t"""
    c = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    He, Hd = X["He"], X["Hd"]
    sh, r = c(X["static_hidden"]), c(X["rnn_out"])
    B, _, nR = sh.shape
    dh = torch.nn.functional.conv1d(c(X["dyn"].astype(np.float32)), c(X["We"])[:, :, None], c(X["be"]))
    enc = torch.cat((sh, dh), 1)
    hidden = torch.cat((enc, r.unsqueeze(2).repeat(1, 1, nR)), 1)
    va, vp = c(X["va"]).view(1, 1, Hd).expand(B, 1, Hd), c(X["vp"]).view(1, 1, Hd).expand(B, 1, Hd)
    Wa, Wp = c(X["Wa"]).unsqueeze(0).expand(B, -1, -1), c(X["Wp"]).unsqueeze(0).expand(B, -1, -1)
    attn = torch.softmax(torch.bmm(va, torch.tanh(torch.bmm(Wa, hidden))), dim=2)
    context = attn.bmm(enc.permute(0, 2, 1))
    energy = torch.cat((enc, context.transpose(1, 2).expand_as(enc)), dim=1)
    logits = torch.bmm(vp, torch.tanh(torch.bmm(Wp, energy))).squeeze(1)
    t = torch.bmm(Wp[:, :, 2 * He:], context.transpose(1, 2)).squeeze(2)
    return logits, attn.squeeze(1), t


def folded_torch(proj, dynf, M, k, q, va, vp):
    """the contract in torch on (B, 3 Hd, nR) proj and a floating 0/1 ``dynf``, differentiable -> logits, attn, t"""
    Hd = q.shape[1]
    U = proj + k[None, :, None] + torch.einsum('xr,brc->bxc', M, dynf)
    attn = torch.softmax(torch.einsum('j,bjc->bc', va, torch.tanh(U[:, :Hd] + q[:, :, None])), dim=1)
    t = torch.einsum('bc,bjc->bj', attn, U[:, 2 * Hd:])
    logits = torch.einsum('j,bjc->bc', vp, torch.tanh(U[:, Hd:2 * Hd] + t[:, :, None]))
    return logits, attn, t


def tolerance(e_ref, want):
    """what a float32 result may be off by: four times the float32 reference's own error -- the device's tanhf / expf are
    a few ulp off and the sums run in another order -- with a floor of 16 ulp of the largest wanted value, so that a
    lucky e_ref does not fail a correct kernel"""
    return 4.0 * e_ref + 16.0 * U32 * float(np.abs(want).max())
