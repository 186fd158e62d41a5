"""The model of dropout inside the decoder step (tapenv.h: tap_decoder_step_dropout), the tests' oracle.

The masks.  Philox4x32-10 with the standard constants; for env b (its index in the call plus env_offset), hidden row j,
decoding step t and episode e the counter is (b, j, t, e mod 2^32) and the key (seed mod 2^32, seed >> 32).  Output word 0
decides drop_rnn, word 1 drop_hh: keep iff word >= thr, thr = min(2^32 - 1, round(p 2^32)).  A kept element is x s with
s = float32(1 / (1 - p)), a dropped one 0.  Packed: (B, 2, Hd / 64) int64, plane 0 drop_rnn, plane 1 drop_hh, bit j mod 64 of
word j / 64 set iff row j is kept.  Everything here is numpy in uint64 -- nothing is shared with the torch form
(rollout.dropout_keep_words) or the kernels.

The step.  decoder_step_model's step with h_out = drop_hh(h') and q = Wq . drop_rnn(h'); the reference's form (the two
nn.Conv1d, nn.GRU) with the same explicit masks gives e_ref.

The training loop.  episode_actor_model.train_step with the pointer's two nn.Dropout replaced by modules that apply the
model's masks for (seed, episode, step): the reference's own ``forward`` then runs with explicit masks, in any dtype."""
import copy

import numpy as np
import torch
from torch import nn

import decoder_step_model as M
import episode_actor_model as A

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter (4 arrays or ints), key (2) of values < 2^32 -> the four output words, uint64 arrays of values < 2^32"""
    c = [np.asarray(v, np.uint64) for v in counter]
    k = [np.asarray(v, np.uint64) for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]         # < 2^64: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return c


def threshold(p):
    return min(2 ** 32 - 1, int(np.floor(p * 2.0 ** 32 + 0.5)))


def scale(p):
    """float32(1 / (1 - p)) as a float64 value"""
    return float(np.float32(1.0 / (1.0 - p)))


def keep_bool(seed, episode, step, B, Hd, p_rnn, p_hh, env_offset=0):
    """-> bool (B, 2, Hd): [:, 0] drop_rnn's keep mask, [:, 1] drop_hh's"""
    b = ((np.arange(B, dtype=np.uint64) + np.uint64(env_offset)) & MASK)[:, None] + np.zeros((1, Hd), np.uint64)
    j = np.arange(Hd, dtype=np.uint64)[None, :] + np.zeros((B, 1), np.uint64)
    w = philox4x32_10((b, j, step & 0xFFFFFFFF, episode & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return np.stack((w[0] >= np.uint64(threshold(p_rnn)), w[1] >= np.uint64(threshold(p_hh))), axis=1)


def pack(keep):
    """bool (B, 2, Hd) -> the packed words (B, 2, Hd / 64) int64"""
    B, _, Hd = keep.shape
    bits = keep.reshape(B, 2, Hd // 64, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(bits, axis=-1).view(np.int64)


def keep_words(seed, episode, step, B, Hd, p_rnn, p_hh, env_offset=0):
    return pack(keep_bool(seed, episode, step, B, Hd, p_rnn, p_hh, env_offset))


def apply(x, kept, p):
    """numpy: a kept element is x s, a dropped one +0"""
    return np.where(kept, x * np.asarray(scale(p), x.dtype), np.zeros((), x.dtype))


def masked(hn, wq, keep, p_rnn, p_hh):
    """what the two dropouts make of a step's h' (B, Hd), numpy in hn's dtype: -> h_out = drop_hh(h'), q = wq . drop_rnn(h')
    (from 0, the Hd terms in ascending order), rnn_out = drop_rnn(h'); ``keep`` bool (B, 2, Hd)"""
    rnn = apply(hn, keep[:, 0], p_rnn)
    wq = np.asarray(wq, hn.dtype)
    q = np.zeros_like(hn)
    for k in range(hn.shape[1]):
        q = q + rnn[:, k:k + 1] * wq[:, k][None, :]
    return apply(hn, keep[:, 1], p_hh), q, rnn


def step(xs, xd, h, P, c, w_hh, b_hh, wq, keep, p_rnn, p_hh, dtype=np.float64):
    """decoder_step_model.step with the masks -> h_out, q, gates (of the step before any mask), rnn_out"""
    hn, _, gates = M.step(xs, xd, h, P, c, w_hh, b_hh, wq, dtype)
    h_out, q, rnn = masked(hn, wq, keep, p_rnn, p_hh)
    return h_out, q, gates, rnn


def _t_apply(x, kept, p):
    return torch.where(kept, x * scale(p), torch.zeros_like(x))


def masked_torch(hn, wq, keep, p_rnn, p_hh):
    """``masked`` in torch, differentiable: where model.py:112-115 has its two nn.Dropout, then the decoder's columns of
    the attention's W -> h_out, q, rnn_out; ``keep`` a bool tensor (B, 2, Hd)"""
    rnn = _t_apply(hn, keep[:, 0], p_rnn)
    return _t_apply(hn, keep[:, 1], p_hh), rnn.matmul(wq.t()), rnn


def step_torch(xs, xd, h, P, c, w_hh, b_hh, wq, keep, p_rnn, p_hh):
    """``step`` in torch, differentiable -> h_out, q, gates, rnn_out"""
    hn, _, gates = M.step_torch(xs, xd, h, P, c, w_hh, b_hh, wq)
    h_out, q, rnn = masked_torch(hn, wq, keep, p_rnn, p_hh)
    return h_out, q, gates, rnn


def reference_form_torch(X, dtype, with_h, keep, p_rnn, p_hh):
    """decoder_step_model.reference_form_torch -- the reference's own modules on the CPU; one layer and one step, so
    rnn_out is last_hh -- with the explicit masks -> h_out, q, rnn_out"""
    hn, _ = M.reference_form_torch(X, dtype, with_h)
    return masked_torch(hn, torch.from_numpy(np.asarray(X["Wq"])).to(dtype), torch.from_numpy(keep), p_rnn, p_hh)


class MaskDrop(nn.Module):
    """stands where the pointer has an nn.Dropout and applies the mask it was last given (any leading axes)"""

    def __init__(self, p):
        super(MaskDrop, self).__init__()
        self.p, self.kept = float(p), None

    def forward(self, x):
        return _t_apply(x, self.kept.to(x.device).expand_as(x), self.p)


def with_dropout(actor, p_rnn, p_hh):
    """a copy of an episode_actor_model.Actor in training mode with the pointer's dropouts at these probabilities"""
    net = copy.deepcopy(actor).train()
    net.pointer.drop_rnn.p, net.pointer.drop_hh.p = float(p_rnn), float(p_hh)
    return net


def train_step(actor, dtype, static, env, tour, adv, ghh, seed, episode, env_offset=0):
    """episode_actor_model.train_step with the model's masks: the teacher-forced loop in ``dtype`` on the CPU through the
    reference's ``forward``, step k drawing the masks of (seed, episode, k) at the probabilities of ``actor``'s two dropouts
    -> tour_logp (B, n) and {parameter name: gradient of L}, float64 numpy"""
    c = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    net = copy.deepcopy(actor).to(dtype).train()
    p_rnn, p_hh = net.pointer.drop_rnn.p, net.pointer.drop_hh.p
    net.pointer.drop_rnn, net.pointer.drop_hh = MaskDrop(p_rnn), MaskDrop(p_hh)
    tour = torch.from_numpy(np.asarray(tour, np.int64))
    B, n = tour.shape
    static_hidden = net.static_encoder(c(static))
    hh = torch.zeros(1, B, net.hidden, dtype=dtype)
    logps = []
    for k in range(n):
        keep = torch.from_numpy(keep_bool(seed, episode, k, B, net.hidden, p_rnn, p_hh, env_offset))
        net.pointer.drop_rnn.kept, net.pointer.drop_hh.kept = keep[:, 0], keep[:, 1]
        dynamic_hidden = net.dynamic_encoder(c(env["dynamic"][k]))
        dec = net.decoder_input(c(env["decoder_static"][k]), c(env["decoder_dynamic"][k]))
        logits, hh = net.pointer(static_hidden, dynamic_hidden, dec, hh)
        logps.append(A.masked_log_softmax(logits, c(env["current_mask"][k])).gather(1, tour[:, k:k + 1]))
    tour_logp = torch.cat(logps, dim=1)
    ((c(adv) * tour_logp.sum(1)).sum() + (hh * c(ghh)).sum()).backward()
    return tour_logp.detach().double().numpy(), A.named_grads(net)
