"""The episode loop around the batched environment -- this package's counterpart of the loop in
the reference's ``DRL.forward`` (model.py:342-515), with the policy network factored out.

The reference interleaves its pointer network with a per-env Python loop and two host<->device
copies per step (model.py:407-465).  Here a step is two kernel launches on the current stream
(precedence update, placement) and nothing leaves the device until the caller asks.
"""
import collections
import math
import struct

import torch

from . import _lib
from .env import BatchedContainer
from .pack import EnvTransition, EpisodeStepper, MaskStepper, NonBinaryDynamic, bits_supported, grad_copies


class TapePolicy(object):
    """Replays a recorded tour (B, steps) -- e.g. the reference actor's greedy choices.  The tour is kept
    step-major, so a step's picks are a contiguous (B,) view: no copy kernel between the steps."""

    def __init__(self, tour):
        self.tour = tour
        self._steps = tour.to(torch.int64).t().contiguous()

    def __call__(self, step, **_):
        return self._steps[step]


class RandomFeasiblePolicy(object):
    """Uniformly random selectable column of ``current_mask``: an exponential race -- the column with the smallest
    Exp(1) draw among the selectable ones, argmax(mask / q) -- which is what torch.multinomial(mask, 1) computes
    after its input checks (three torch ops on buffers the policy keeps, instead of ~85 us of host per
    torch.multinomial call on this stack).  Where NO column is selectable argmax returns column 0 (torch.multinomial
    raises there): ``strict=True`` checks for that, at one host sync per call; a recorded run checks the tour against
    the masks afterwards (tests), a trainer's episodes end before the mask empties."""

    def __init__(self, generator=None, strict=False):
        self.generator = generator
        self.strict = strict          # True: raise when an env has no selectable column, as torch.multinomial does (one host sync per call)
        self._q = self._r = None

    def __call__(self, step, current_mask, **_):
        if self.strict and not bool((current_mask.sum(1) > 0).all()):
            raise RuntimeError("RandomFeasiblePolicy: an env has no selectable column (current_mask is all zero there); "
                               "argmax would return column 0")
        if self._q is None or self._q.shape != current_mask.shape or self._q.device != current_mask.device:
            self._q = torch.empty_like(current_mask)
            self._r = torch.empty_like(current_mask)
        self._q.exponential_(generator=self.generator)
        torch.div(current_mask, self._q, out=self._r)
        return torch.argmax(self._r, dim=1)


class MultinomialPolicy(object):
    """The same distribution through torch.multinomial on ``current_mask`` (round 3's stand-in policy)."""

    def __init__(self, generator=None):
        self.generator = generator

    def __call__(self, step, current_mask, **_):
        return torch.multinomial(current_mask, 1, generator=self.generator).squeeze(1)


class UniformPickPolicy(object):
    """Uniformly random selectable column from PRE-DRAWN uniforms ``u`` (B, steps) in [0, 1): the k-th selectable
    column of ``current_mask`` with k = floor(u * count), by cumulative sum -- plain deterministic torch ops, so
    an episode with this policy can be captured in a HIP graph and replayed on refreshed ``u`` (torch's own
    in-graph RNG, ``torch.multinomial`` with a graph-registered generator, aborted under back-to-back replays on
    this ROCm stack)."""

    def __init__(self, u):
        self.u = u

    def __call__(self, step, current_mask, **_):
        cnt = current_mask.sum(1)
        k = torch.minimum((self.u[:, step] * cnt).floor(), cnt - 1).clamp_(min=0)
        return (current_mask.cumsum(1) > k.unsqueeze(1)).to(torch.float32).argmax(1)


class UniformKeysPolicy(object):
    """Uniformly random selectable column from PRE-DRAWN iid keys ``v`` (steps, B, nR) in [0, 1): the selectable
    column with the largest key -- the argmax of iid keys over a set is uniform over the set.  Two torch ops per step
    (a multiply and an argmax), deterministic given ``v``, so an episode with it can be captured in a HIP graph and
    replayed on refreshed keys.  (A key of exactly 0 on the only selectable column would tie with the masked ones;
    torch.rand draws from [0, 1), so add a tiny offset when that matters.)"""

    def __init__(self, v):
        self.v = v

    def __call__(self, step, current_mask, **_):
        return torch.argmax(current_mask * self.v[step], dim=1)


class BestRatioPolicy(object):
    """The greedy best-ratio order (the reference's generate_order_graph(..., find_order_type='best'),
    generate.py:1242-1292): the selectable column whose placement leaves ``env`` -- the container the episode steps --
    with the largest calc_ratio, the first of them on a tie, compared in fp64.  One ``env.trial_scores`` call per step
    on buffers the policy keeps: one launch for the lane-per-cell LB_GREEDY shapes, no host read, so an episode with it
    can be captured in a hipGraph (the other strategies and sizes go through trial_scores' stepped form).
    ``fresh_first``: score step 0 against an empty container -- the fused stepper clears the container inside its
    first step, not before it; pass False when the episode goes on with the container as it is.  After a call
    ``scores`` (B, nR) float64 holds that step's trial scores."""

    def __init__(self, env, fresh_first=True):
        self.env = env
        self.fresh_first = bool(fresh_first)
        self.scores = None
        self._best = []                  # one (B,) buffer per step index: a loop may keep every step's picks as views

    def __call__(self, step, static, current_mask, **_):
        env = self.env
        if int(static.shape[1]) != 1 + env.block_dim:
            raise NotImplementedError("BestRatioPolicy scores one target container: the two-container input types "
                                      "('mul', 'mul-with') are not implemented")
        nR = int(static.shape[2])
        if self.scores is None or tuple(self.scores.shape) != (env.batch_size, nR):
            self.scores = torch.empty(env.batch_size, nR, dtype=torch.float64, device=env.device)
        while len(self._best) <= step:
            self._best.append(torch.empty(env.batch_size, dtype=torch.int64, device=env.device))
        best = self._best[step]
        env.trial_scores(static, current_mask, fresh=self.fresh_first and step == 0, out=self.scores, best_out=best)
        return best


def _prep_f32(t, dev):
    """``t`` as a contiguous float32 tensor on ``dev`` (None stays None); the cast is ``.float()``, so autograd sees it"""
    if t is None:
        return None
    if t.dtype is not torch.float32:
        t = t.float()
    if not t.is_contiguous() or t.device != dev:
        t = t.to(dev).contiguous()
    return t


def _pick_into(logits, mask, u, ptr, logp, probs):
    """tap_policy_pick on prepared buffers: one launch on the current stream, nothing allocated"""
    dev = logits.device
    c = _lib.ctx(dev)
    B, nR = int(logits.shape[0]), int(logits.shape[1])
    _lib.check(_lib.lib().tap_policy_pick(c, _lib.ptr(logits), _lib.ptr(mask), _lib.ptr(u), B, nR,
                                          _lib.TAP_P_GREEDY if u is None else 0, _lib.ptr(ptr), _lib.ptr(logp),
                                          _lib.ptr(probs), _lib.stream_of(dev)), c)


class _PointerPick(torch.autograd.Function):
    """pointer_pick under autograd: forward = the head's launch with probs kept, backward = tap_policy_pick_backward.
    probs is the head's OWN output: the stepper's mask buffers alternate and are overwritten two steps later, so the
    mask is not what backward keeps."""

    @staticmethod
    def forward(ctx, logits, mask, u):
        B, nR = logits.shape
        ptr = torch.empty(B, dtype=torch.int64, device=logits.device)
        logp = torch.empty(B, dtype=torch.float32, device=logits.device)
        probs = torch.empty(B, nR, dtype=torch.float32, device=logits.device)
        _pick_into(logits, mask, u, ptr, logp, probs)
        ctx.save_for_backward(probs, ptr, logp)
        ctx.mark_non_differentiable(ptr, probs)
        return ptr, logp, probs

    @staticmethod
    def backward(ctx, _g_ptr, g, _g_probs):
        probs, ptr, logp = ctx.saved_tensors
        g = _prep_f32(g, probs.device)
        B, nR = probs.shape
        out = torch.empty_like(probs)
        c = _lib.ctx(probs.device)
        _lib.check(_lib.lib().tap_policy_pick_backward(c, _lib.ptr(probs), _lib.ptr(ptr), _lib.ptr(logp), _lib.ptr(g), int(B),
                                                       int(nR), _lib.ptr(out), _lib.stream_of(probs.device)), c)
        return out, None, None


def pointer_pick(logits, mask, u=None, want_probs=False):
    """The decoding head (tapenv.h: tap_policy_pick; model.py:359-372): masked softmax, pick and log-probability in ONE
    launch.  ``logits`` (B, nR) from the pointer network, ``mask`` (B, nR) the stepper's ``current_mask`` (a column is
    selectable iff mask != 0; logits on unselectable columns are never used, NaN and +-inf included; logits on
    selectable columns must be finite), ``u`` (B,) uniforms in [0, 1) to sample with, or None for the greedy pick (the
    first selectable column holding the row's maximum).  -> (ptr (B,) int64, logp (B,) float32[, probs (B, nR)
    float32 with ``want_probs``]).  Sampling takes the first selectable column whose inclusive prefix sum of
    exp(l - max) exceeds u * sum, in fp64: an unselectable column is never returned, so there is no rejection loop and
    no host read.  A row with no selectable column gives ptr 0, logp NaN, probs 0.
    Tensors of another dtype, layout or device are converted as ``BatchedContainer.trial_scores`` converts its inputs
    (half / bf16 logits through ``.float()``, so autograd sees the cast).  With grad enabled and
    ``logits.requires_grad``, ``logp`` carries its gradient to ``logits`` through one backward launch
    (-g * probs off the pick, the picked column minus the sum of the others so that a row sums to zero, zeros on rows whose
    logp is NaN); ``ptr`` and ``probs`` are not differentiable."""
    if logits.dim() != 2 or int(logits.shape[1]) < 1:
        raise ValueError("logits must be (B, nR) with nR >= 1, got %s" % (tuple(logits.shape),))
    dev = _lib.resolve_device(logits.device)
    B, nR = int(logits.shape[0]), int(logits.shape[1])
    if tuple(mask.shape) != (B, nR):
        raise ValueError("mask must be (%d, %d), got %s" % (B, nR, tuple(mask.shape)))
    if u is not None and tuple(u.shape) != (B,):
        raise ValueError("u must be (%d,), got %s" % (B, tuple(u.shape)))
    logits = _prep_f32(logits, dev)
    mask = _prep_f32(mask.detach(), dev)
    u = None if u is None else _prep_f32(u.detach(), dev)
    if torch.is_grad_enabled() and logits.requires_grad:
        ptr, logp, probs = _PointerPick.apply(logits, mask, u)
    else:
        ptr = torch.empty(B, dtype=torch.int64, device=dev)
        logp = torch.empty(B, dtype=torch.float32, device=dev)
        probs = torch.empty(B, nR, dtype=torch.float32, device=dev) if want_probs else None
        _pick_into(logits, mask, u, ptr, logp, probs)
    return (ptr, logp, probs) if want_probs else (ptr, logp)


PickRecord = collections.namedtuple("PickRecord", "state step env_offset")
PickRecord.__doc__ = """what a DRAW pick takes: ``state`` the int64[2] (seed, episode) tensor, ``step`` the decoding step (a Python
int) and the index of the call's first env in the whole batch (``tools.StepDropout.take_pick``)"""

PICK_ROW = 0xFFFFFFFF          # the hidden row of the pick's Philox counter: no dropout launch has it


def _pick_record(source):
    """-> a checked PickRecord from a ``tools.StepDropout`` (its next pick), a record or a plain (state, step[, env_offset])"""
    if hasattr(source, "take_pick"):
        source = source.take_pick()
    d = PickRecord(*source) if len(source) == 3 else PickRecord(*source, 0)
    if not torch.is_tensor(d.state) or d.state.dtype is not torch.int64 or tuple(d.state.shape) != (2,) or not d.state.is_contiguous():
        raise ValueError("the pick's state must be a contiguous int64[2] (seed, episode) tensor")
    if int(d.step) < 0 or int(d.env_offset) < 0:
        raise ValueError("the pick's step and env_offset must not be negative, got %r and %r" % (d.step, d.env_offset))
    return d


def pick_uniforms(state, step, B, env_offset=0):
    """The uniforms of a DRAW pick in torch integer ops (tapenv.h: tap_policy_pick_draw) -> (B,) float32 on ``state``'s
    device: Philox4x32-10 at counter (env_offset + b, 0xFFFFFFFF, step, episode mod 2^32) and key (seed mod 2^32, seed >> 32),
    u = (word0 >> 8) * 2^-24.  It reads no value on the host."""
    dev = state.device
    seed, episode = state[0], state[1]
    env = (torch.arange(int(B), dtype=torch.int64, device=dev) + int(env_offset)) & _M32
    zero = torch.zeros_like(env)
    w = philox4x32_10((env, zero + PICK_ROW, zero + (int(step) & _M32), zero + (episode & _M32)), (seed & _M32, (seed >> 32) & _M32))
    return (w[0] >> 8).to(torch.float32) * (2.0 ** -24)


def _pick_draw_into(logits, mask, rec, ptr, logp, probs, u):
    """tap_policy_pick_draw on prepared buffers: one launch on the current stream, nothing allocated"""
    dev = logits.device
    if rec.state.device != dev:
        raise ValueError("the pick's state lives on %s, the logits on %s: the launch reads the state on its own device"
                         % (rec.state.device, dev))
    c = _lib.ctx(dev)
    B, nR = int(logits.shape[0]), int(logits.shape[1])
    _lib.check(_lib.lib().tap_policy_pick_draw(c, _lib.ptr(logits), _lib.ptr(mask), _lib.ptr(rec.state), int(rec.step) & _M32,
                                               int(rec.env_offset) & _M32, B, nR, _lib.ptr(ptr), _lib.ptr(logp), _lib.ptr(probs),
                                               _lib.ptr(u), _lib.stream_of(dev)), c)


def _pick_given_into(logits, mask, ptr_in, logp, probs):
    """tap_policy_pick_given on prepared buffers: one launch on the current stream, nothing allocated"""
    dev = logits.device
    c = _lib.ctx(dev)
    B, nR = int(logits.shape[0]), int(logits.shape[1])
    _lib.check(_lib.lib().tap_policy_pick_given(c, _lib.ptr(logits), _lib.ptr(mask), _lib.ptr(ptr_in), B, nR, _lib.ptr(logp),
                                                _lib.ptr(probs), _lib.stream_of(dev)), c)


class _PointerPickDraw(torch.autograd.Function):
    """pointer_pick_draw under autograd: forward = the DRAW launch with probs kept, backward = ``_PointerPick``'s"""

    @staticmethod
    def forward(ctx, logits, mask, rec, want_u):
        B, nR = logits.shape
        ptr = torch.empty(B, dtype=torch.int64, device=logits.device)
        logp = torch.empty(B, dtype=torch.float32, device=logits.device)
        probs = torch.empty(B, nR, dtype=torch.float32, device=logits.device)
        u = torch.empty(B, dtype=torch.float32, device=logits.device) if want_u else None
        _pick_draw_into(logits, mask, rec, ptr, logp, probs, u)
        ctx.save_for_backward(probs, ptr, logp)
        ctx.mark_non_differentiable(*(t for t in (ptr, probs, u) if t is not None))
        return ptr, logp, probs, u

    @staticmethod
    def backward(ctx, _g_ptr, g, _g_probs, _g_u):
        return _PointerPick.backward(ctx, None, g, None)[0], None, None, None


class _PointerPickGiven(torch.autograd.Function):
    """pointer_pick_given under autograd: forward = the GIVEN launch with probs kept, backward = ``_PointerPick``'s on the
    caller's column (a CLONE of it: a stepper's tour buffer is overwritten by the next episode)"""

    @staticmethod
    def forward(ctx, logits, mask, ptr_in):
        B, nR = logits.shape
        logp = torch.empty(B, dtype=torch.float32, device=logits.device)
        probs = torch.empty(B, nR, dtype=torch.float32, device=logits.device)
        _pick_given_into(logits, mask, ptr_in, logp, probs)
        ctx.save_for_backward(probs, ptr_in.clone(), logp)
        ctx.mark_non_differentiable(probs)
        return logp, probs

    @staticmethod
    def backward(ctx, g, _g_probs):
        return _PointerPick.backward(ctx, None, g, None)[0], None, None


def _pick_inputs(logits, mask):
    """the checks and conversions of ``pointer_pick`` -> logits, mask (float32, contiguous, on the device), B, nR, dev"""
    if logits.dim() != 2 or int(logits.shape[1]) < 1:
        raise ValueError("logits must be (B, nR) with nR >= 1, got %s" % (tuple(logits.shape),))
    dev = _lib.resolve_device(logits.device)
    B, nR = int(logits.shape[0]), int(logits.shape[1])
    if tuple(mask.shape) != (B, nR):
        raise ValueError("mask must be (%d, %d), got %s" % (B, nR, tuple(mask.shape)))
    return _prep_f32(logits, dev), _prep_f32(mask.detach(), dev), B, nR, dev


def pointer_pick_draw(logits, mask, source, want_probs=False, want_u=False):
    """``pointer_pick``'s sampling with the uniforms computed INSIDE the launch (tapenv.h: tap_policy_pick_draw): ``source`` is
    a ``tools.StepDropout`` -- the call takes its next pick record --, a ``PickRecord`` or a plain (state, step[, env_offset])
    with ``state`` the int64[2] (seed, episode) on the logits' device.  Counter-based: a row's pick depends on (seed, episode,
    step, env_offset + b) and the row alone -- not on the batch size, the launch or torch's generator --, and a captured
    episode draws anew on every replay once ``next_episode()`` is captured at its head.  -> (ptr, logp[, probs][, u]); ``u``
    (B,) float32 is what the launch drew: ``pointer_pick(logits, mask, u)`` returns the same bytes.  Autograd as
    ``pointer_pick``."""
    logits, mask, B, nR, dev = _pick_inputs(logits, mask)
    rec = _pick_record(source)
    if torch.is_grad_enabled() and logits.requires_grad:
        ptr, logp, probs, u = _PointerPickDraw.apply(logits, mask, rec, bool(want_u))
    else:
        ptr = torch.empty(B, dtype=torch.int64, device=dev)
        logp = torch.empty(B, dtype=torch.float32, device=dev)
        probs = torch.empty(B, nR, dtype=torch.float32, device=dev) if want_probs else None
        u = torch.empty(B, dtype=torch.float32, device=dev) if want_u else None
        _pick_draw_into(logits, mask, rec, ptr, logp, probs, u)
    return (ptr, logp) + ((probs,) if want_probs else ()) + ((u,) if want_u else ())


def pointer_pick_given(logits, mask, ptr, want_probs=False):
    """The log-probability of GIVEN columns ``ptr`` (B,) int64 under the head's masked softmax, in one launch (tapenv.h:
    tap_policy_pick_given): teacher forcing, or old tours under new weights.  -> logp (B,) float32[, probs (B, nR)]; NaN where
    ``ptr`` lies outside [0, nR) or on an unselectable column.  With ``ptr`` what ``pointer_pick`` returned for the same
    inputs, ``logp`` and ``probs`` are that call's bytes.  Autograd as ``pointer_pick`` (a NaN row has a zero gradient)."""
    logits, mask, B, nR, dev = _pick_inputs(logits, mask)
    if tuple(ptr.shape) != (B,) or ptr.is_floating_point():
        raise ValueError("ptr must be an integer (%d,) tensor, got %s %s" % (B, ptr.dtype, tuple(ptr.shape)))
    if ptr.dtype is not torch.int64 or not ptr.is_contiguous() or ptr.device != dev:
        ptr = ptr.to(device=dev, dtype=torch.int64).contiguous()
    if torch.is_grad_enabled() and logits.requires_grad:
        logp, probs = _PointerPickGiven.apply(logits, mask, ptr)
    else:
        logp = torch.empty(B, dtype=torch.float32, device=dev)
        probs = torch.empty(B, nR, dtype=torch.float32, device=dev) if want_probs else None
        _pick_given_into(logits, mask, ptr, logp, probs)
    return (logp, probs) if want_probs else logp


def pointer_pick_torch(logits, mask, u=None, given=None):
    """The head in torch ops, float64, for tensors off the GPU (``tools.DRL``'s fallback; the kernels' definition, tapenv.h:
    tap_policy_pick): ``given`` (B,) int64 scores those columns, else ``u`` (B,) samples and None picks greedily.  -> (ptr,
    logp in the dtype of ``logits``); differentiable in ``logits``."""
    sel = mask != 0
    l = torch.where(sel, logits.double(), torch.full_like(logits, float('-inf'), dtype=torch.float64))
    any_ = sel.any(1)
    m = torch.where(any_, l.max(1).values, torch.zeros_like(l[:, 0]))
    w = torch.where(sel, torch.exp(l - m.unsqueeze(1)), torch.zeros_like(l))
    S = w.sum(1)
    nR = int(logits.shape[1])
    if given is not None:
        ptr = given.to(torch.int64)
        ok = (ptr >= 0) & (ptr < nR)
        at = ptr.clamp(0, nR - 1)
        ok = ok & sel.gather(1, at.unsqueeze(1))[:, 0]
    else:
        if u is None:
            hit = sel & (l == m.unsqueeze(1))
        else:
            hit = sel & (w.cumsum(1) > (u.double() * S).unsqueeze(1))
        cols = torch.arange(nR, device=logits.device).unsqueeze(0)
        first = torch.where(hit, cols, torch.full_like(cols, nR)).min(1).values
        last = torch.where(sel, cols, torch.zeros_like(cols)).max(1).values
        ptr = at = torch.where(first < nR, first, last)
        ok = any_
    # the unselectable columns hold -inf: a picked column is selectable, and gather's gradient reaches that column alone
    l_ptr = torch.where(ok, l.gather(1, at.unsqueeze(1))[:, 0], torch.zeros_like(m))
    logp = torch.where(ok, (l_ptr - m) - torch.log(torch.where(ok, S, torch.ones_like(S))), torch.full_like(m, float('nan')))
    return ptr, logp.to(logits.dtype)


def _encode_into(bits, weight, bias, rows, out):
    """tap_encode_bits on prepared buffers: one launch on the current stream, nothing allocated"""
    dev = bits.device
    c = _lib.ctx(dev)
    B, H, nR = (int(v) for v in out.shape)
    _lib.check(_lib.lib().tap_encode_bits(c, _lib.ptr(bits), B, nR, rows, H, _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out),
                                          _lib.stream_of(dev)), c)


class _EncodeBits(torch.autograd.Function):
    """encode_dynamic_bits under autograd: forward = the encoder's launch, backward = tap_encode_bits_backward (two
    launches, the scratch from torch.empty).  What backward keeps is the SHADOW, B * words * 8 bytes, not an fp32
    tensor -- and a CLONE of it: the stepper's shadow buffers alternate and are overwritten two steps later, long
    before an episode's backward runs."""

    @staticmethod
    def forward(ctx, bits, weight, bias, rows, nR):
        B, H = int(bits.shape[0]), int(weight.shape[0])
        out = torch.empty(B, H, nR, dtype=torch.float32, device=bits.device)
        _encode_into(bits, weight, bias, rows, out)
        ctx.save_for_backward(bits.clone())
        ctx.shape = (B, nR, rows, H)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        bits, = ctx.saved_tensors
        B, nR, rows, H = ctx.shape
        dev = bits.device
        g = _prep_f32(g, dev)
        L, c = _lib.lib(), _lib.ctx(dev)
        dweight = torch.empty(H, rows, dtype=torch.float32, device=dev)
        dbias = torch.empty(H, dtype=torch.float32, device=dev) if ctx.has_bias and ctx.needs_input_grad[2] else None
        if B == 0:
            dweight.zero_()
            if dbias is not None:
                dbias.zero_()
            return None, dweight, dbias, None, None
        need = int(L.tap_encode_bits_backward_scratch(B, nR, rows, H))
        scratch = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=dev)
        _lib.check(L.tap_encode_bits_backward(c, _lib.ptr(bits), _lib.ptr(g), B, nR, rows, H, _lib.ptr(dweight), _lib.ptr(dbias),
                                              _lib.ptr(scratch), need, _lib.stream_of(dev)), c)
        return None, dweight, dbias, None, None


def encode_dynamic_bits(bits, weight, bias=None, rows=None):
    """The dynamic encoder on the bit shadow (tapenv.h: tap_encode_bits; model.py:380, dynamic_encoder(dynamic)): the 1x1
    convolution of the 0/1 tensor ``dynamic`` computed from its shadow in ONE launch -> (B, H, nR) float32.
    ``bits`` int64 in ``pack.dynamic_bits`` layout, (B, nR) -- (B, 2 * nR) or (B, 2, nR) above 64 rows (a stepper's
    ``dynamic_bits``); ``weight`` (H, rows) or (H, rows, 1) = Conv1d.weight; ``bias`` (H,) or None; ``rows`` defaults to
    ``weight.shape[1]`` (bits at positions >= rows are ignored).  out[b, h, c] = bias[h] + the W[h, r] of the rows r set
    in column c, added in ascending row order in fp32: no multiplication, reproducible bit for bit.
    ``weight`` / ``bias`` of another dtype, layout or device are converted as ``pointer_pick`` converts its logits (through
    ``.float()``, so autograd sees the cast).  With grad enabled and ``weight`` or ``bias`` requiring grad the call runs
    through a ``torch.autograd.Function`` whose backward is tap_encode_bits_backward (deterministic: no atomics); it keeps
    a clone of ``bits`` (B * words * 8 bytes), never an fp32 ``dynamic``.  The bits carry no gradient."""
    if bits.dtype is not torch.int64:
        raise TypeError("bits must be the int64 shadow (pack.dynamic_bits), got %s" % (bits.dtype,))
    if weight.dim() == 3 and int(weight.shape[2]) == 1:
        weight = weight.squeeze(2)
    if weight.dim() != 2 or not weight.is_floating_point():
        raise ValueError("weight must be a floating (H, rows) or (H, rows, 1) tensor, got %s %s" % (weight.dtype, tuple(weight.shape)))
    H = int(weight.shape[0])
    rows = int(weight.shape[1]) if rows is None else int(rows)
    if rows != int(weight.shape[1]):
        raise ValueError("weight has %d input rows, rows is %d" % (int(weight.shape[1]), rows))
    if bits.dim() not in (2, 3) or rows < 1:
        raise ValueError("bits must be (B, words) or (B, planes, nR), got %s" % (tuple(bits.shape),))
    B = int(bits.shape[0])
    planes = 2 if rows > 64 else 1
    words = int(math.prod(bits.shape[1:]))
    nR = words // planes
    if words != planes * nR or nR < 1 or (bits.dim() == 3 and tuple(bits.shape[1:]) != (planes, nR)):
        raise ValueError("bits of shape %s is not the shadow of a window of %d rows (%d plane(s))" % (tuple(bits.shape), rows, planes))
    if not (1 <= H <= 1024) or _lib.lib().tap_bits_words(rows, nR) != words:
        raise ValueError("no bit shadow / encoder for rows %d, nR %d, H %d (rows <= 128, nR %% 4 == 0, nR <= 256, H <= 1024)" % (rows, nR, H))
    if bias is not None and (tuple(bias.shape) != (H,) or not bias.is_floating_point()):
        raise ValueError("bias must be a floating (%d,) tensor, got %s %s" % (H, bias.dtype, tuple(bias.shape)))
    dev, bits = _bits_on_device(bits)
    weight = _prep_f32(weight, dev)
    bias = _prep_f32(bias, dev)
    if torch.is_grad_enabled() and (weight.requires_grad or (bias is not None and bias.requires_grad)):
        return _EncodeBits.apply(bits, weight, bias, rows, nR)
    out = torch.empty(B, H, nR, dtype=torch.float32, device=dev)
    _encode_into(bits, weight.detach(), None if bias is None else bias.detach(), rows, out)
    return out


def pointer_scores_supported(rows, nR, Hd):
    """whether tap_pointer_scores has a kernel for this shape: a window with a shadow and Hd 64, 128 or 256"""
    return int(Hd) in (64, 128, 256) and _lib.lib().tap_bits_words(int(rows), int(nR)) > 0


def _bits_on_device(bits):
    """-> (the device the launch runs on, the shadow contiguous on it)"""
    dev = _lib.resolve_device(bits.device)
    if not bits.is_contiguous() or bits.device != dev:
        bits = bits.to(dev).contiguous()
    return dev, bits


def _shadow_inputs(bits, name, lead, M, rows, named, blocks=None):
    """The shared opening of the wrappers on the bit shadow.  ``lead`` gives the batch and the window: ``proj`` (B, 3, nR, Hd)
    (``name`` "proj"), the pointer's ``xs`` (B, S, nR) or the critic's ``x`` (B, S, nR); ``M`` (3 Hd, rows) -- the critic's
    (H, rows) -- gives the hidden size and ``rows``; ``named(B, S, nR, Hd)`` lists the other tensors as (name, tensor, the shapes
    it may have).  -> (B, S, nR, Hd or H, rows); S = 0 for ``proj``.  No device is touched: ``_bits_on_device`` follows, after the
    caller's own refusals"""
    if bits.dtype is not torch.int64:
        raise TypeError("bits must be the int64 shadow (pack.dynamic_bits), got %s" % (bits.dtype,))
    if name == "proj":
        if lead.dim() != 4 or int(lead.shape[1]) != 3 or not lead.is_floating_point():
            raise ValueError("proj must be a floating (B, 3, nR, Hd) tensor, got %s %s" % (lead.dtype, tuple(lead.shape)))
        (B, _, nR, Hd), S = (int(v) for v in lead.shape), 0
        m_ok, m_shape = M.dim() == 2 and int(M.shape[0]) == 3 * Hd, "(%d, rows)" % (3 * Hd)
    else:
        if lead.dim() != 3 or not lead.is_floating_point():
            raise ValueError("%s must be a floating (B, S, nR) tensor, got %s %s" % (name, lead.dtype, tuple(lead.shape)))
        B, S, nR = (int(v) for v in lead.shape)
        if name == "xs" and not 1 <= S <= 8:
            raise ValueError("xs has %d static rows; the kernel takes 1 .. 8" % S)
        seg = 3 if name == "xs" else 1
        m_ok, m_shape = M.dim() == 2 and int(M.shape[0]) % seg == 0, "(3 Hd, rows)" if seg == 3 else "(H, rows)"
        Hd = int(M.shape[0]) // seg if m_ok else 0
    if not m_ok or not M.is_floating_point():
        raise ValueError("M must be a floating %s tensor, got %s %s" % (m_shape, M.dtype, tuple(M.shape)))
    rows = int(M.shape[1]) if rows is None else int(rows)
    if rows != int(M.shape[1]):
        raise ValueError("M has %d rows' columns, rows is %d" % (int(M.shape[1]), rows))
    for nm, v, *shapes in named(B, S, nR, Hd):
        if tuple(v.shape) not in shapes or not v.is_floating_point():
            raise ValueError("%s must be a floating %s tensor, got %s %s" % (nm, " or ".join(str(s) for s in shapes), v.dtype,
                                                                           tuple(v.shape)))
    planes = 2 if rows > 64 else 1
    bits_ok = bits.dim() in (2, 3) and int(bits.shape[0]) == B and int(math.prod(bits.shape[1:])) == planes * nR and \
        (bits.dim() == 2 or tuple(bits.shape[1:]) == (planes, nR))
    # the static-rows forms name a wrong shadow before a shape without a kernel, the other two the other way round
    if name == "xs" and not bits_ok:
        raise ValueError("xs of shape %s and bits of shape %s are not (B, S, nR) and the shadow of B envs of a (%d, nR) window"
                         % (tuple(lead.shape), tuple(bits.shape), rows))
    if name == "x":
        if rows < 1 or nR < 1 or not critic_value_supported(rows, nR, Hd, S, blocks):
            raise ValueError("no critic kernel for rows %d, nR %d, H %d, S %d, blocks %d (rows <= 128, nR %% 4 == 0, nR <= 256, "
                             "H 64 / 128 / 256, S 1..8, blocks 1..8)" % (rows, nR, Hd, S, blocks))
    elif rows < 1 or nR < 1 or not pointer_scores_supported(rows, nR, Hd):   # (S is 1 .. 8 or the proj form's 0 here)
        raise ValueError("no pointer kernel for rows %d, nR %d, Hd %d%s (rows <= 128, nR %% 4 == 0, nR <= 256, Hd 64 / 128 / 256%s)"
                         % ((rows, nR, Hd) + ((", S %d" % S, ", S <= 8") if S else ("", ""))))
    if not bits_ok:
        raise ValueError("bits of shape %s is not the shadow of %d envs of a (%d, %d) window" % (tuple(bits.shape), B, rows, nR))
    return B, S, nR, Hd, rows


def _scores_outputs(B, nR, Hd, dev):
    """logits (B, nR), attn (B, nR), t (B, Hd): what the pointer's forward launches write"""
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    return f(B, nR), f(B, nR), f(B, Hd)


def _backward_on_bits(bits, rows, dU, dM, dk, need, launch):
    """The second half of the backwards on the bit shadow: ``launch(ctx, scratch pointer, need, stream)`` is the kernel's own
    backward, which writes dU (B, X, nR) with ``need`` bytes of scratch; then tap_encode_bits_backward on dU, the encoder's backward
    with H = X: dM[x, r] = sum over (b, c) of dU[b, x, c] bit[b, r, c], dk[x] = sum of dU.  One scratch serves both."""
    B, X, nR = (int(v) for v in dU.shape)
    dev = dU.device
    L, c, st = _lib.lib(), _lib.ctx(dev), _lib.stream_of(dev)
    need2 = int(L.tap_encode_bits_backward_scratch(B, nR, rows, X))
    scratch = torch.empty(max(need, need2, 16) // 4, dtype=torch.float32, device=dev)
    _lib.check(launch(c, _lib.ptr(scratch), need, st), c)
    _lib.check(L.tap_encode_bits_backward(c, _lib.ptr(bits), _lib.ptr(dU), B, nR, rows, X, _lib.ptr(dM), _lib.ptr(dk),
                                          _lib.ptr(scratch), need2, st), c)


def _pointer_backward(lead, static, bits, M, k, q, va, vp, attn, t, g, rows):
    """The pointer's backward for both forms: ``static`` None -- ``lead`` is proj, tap_pointer_scores_backward -- or (G, g) --
    ``lead`` is xs, tap_pointer_scores_static_backward --, then ``_backward_on_bits``.  -> dU (B, 3 Hd, nR), dq, dva, dvp, dM, dk;
    an empty batch gives zeros for the parameters' gradients"""
    B, nR, Hd = int(lead.shape[0]), int(attn.shape[1]), int(q.shape[1])
    dev = lead.device
    p, L = _lib.ptr, _lib.lib()
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    dU, dq, dva, dvp, dM, dk = f(B, 3 * Hd, nR), f(B, Hd), f(Hd), f(Hd), f(3 * Hd, rows), f(3 * Hd)
    if B == 0:
        for z in (dva, dvp, dM, dk):
            z.zero_()
        return dU, dq, dva, dvp, dM, dk
    g = _prep_f32(g, dev)
    common = (p(M), p(k), p(q), p(va), p(vp), p(attn), p(t), p(g), p(dU), p(dq), p(dva), p(dvp))
    if static is None:
        need = int(L.tap_pointer_scores_backward_scratch(B, nR, rows, Hd))
        launch = lambda c, scratch, n, st: L.tap_pointer_scores_backward(c, p(lead), p(bits), B, nR, rows, Hd, *common, scratch, n, st)
    else:
        S = int(lead.shape[1])
        need = int(L.tap_pointer_scores_static_backward_scratch(B, nR, rows, Hd, S))
        launch = lambda c, scratch, n, st: L.tap_pointer_scores_static_backward(c, p(lead), p(bits), B, nR, rows, Hd, S, p(static[0]),
                                                                                p(static[1]), *common, scratch, n, st)
    _backward_on_bits(bits, rows, dU, dM, dk, need, launch)
    return dU, dq, dva, dvp, dM, dk


def _scores_into(proj, bits, M, k, q, va, vp, rows, logits, attn, t):
    """tap_pointer_scores on prepared buffers: one launch on the current stream, nothing allocated"""
    dev = proj.device
    c = _lib.ctx(dev)
    B, _, nR, Hd = (int(v) for v in proj.shape)
    _lib.check(_lib.lib().tap_pointer_scores(c, _lib.ptr(proj), _lib.ptr(bits), B, nR, rows, Hd, _lib.ptr(M), _lib.ptr(k),
                                             _lib.ptr(q), _lib.ptr(va), _lib.ptr(vp), _lib.ptr(logits), _lib.ptr(attn),
                                             _lib.ptr(t), _lib.stream_of(dev)), c)


class _PointerScores(torch.autograd.Function):
    """pointer_scores under autograd: forward = the one launch, backward = tap_pointer_scores_backward (dU, dq, dva, dvp)
    and tap_encode_bits_backward on dU (dM, dk).  What a step keeps beside its inputs: a CLONE of the shadow (the
    stepper's shadow buffers alternate and are overwritten two steps later), attn (B, nR), t and q (B, Hd) -- nothing of
    size Hd * nR per env; ``proj`` is the episode's one tensor, kept by reference."""

    @staticmethod
    def forward(ctx, proj, bits, M, k, q, va, vp, rows):
        B, _, nR, Hd = (int(v) for v in proj.shape)
        logits, attn, t = _scores_outputs(B, nR, Hd, proj.device)
        _scores_into(proj, bits, M, k, q, va, vp, rows, logits, attn, t)
        ctx.save_for_backward(proj, bits.clone(), M, k, q, va, vp, attn, t)
        ctx.rows = rows
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        proj, bits, *rest = ctx.saved_tensors
        dU, dq, dva, dvp, dM, dk = _pointer_backward(proj, None, bits, *rest, g, ctx.rows)
        B, Hd3, nR = dU.shape
        # dproj is dU read in proj's layout (B, 3, nR, Hd): a view, not a copy
        return dU.view(B, 3, Hd3 // 3, nR).transpose(2, 3), None, dM, dk, dq, dva, dvp, None


def pointer_scores(proj, bits, M, k, q, va, vp, rows=None):
    """The pointer network's glimpse and logits on the bit shadow (tapenv.h: tap_pointer_scores; model.py:38-138 after
    the GRU step) in ONE launch -> logits (B, nR) float32, the reference's ``probs`` before the head.
    ``proj`` (B, 3, nR, Hd): the per-episode projection of static_hidden, segment-major and hidden fastest
    (``tools.Pointer.project_static`` builds it); ``bits`` int64 in ``pack.dynamic_bits`` layout, (B, nR) -- (B, 2 * nR) or
    (B, 2, nR) above 64 rows; ``M`` (3 Hd, rows) and ``k`` (3 Hd,) the dynamic encoder folded into the two W; ``q`` (B, Hd)
    the decoder's part of the attention; ``va`` / ``vp`` (Hd,) the two v.  ``rows`` defaults to ``M.shape[1]``; bits at
    positions >= rows are ignored.  Per env and column, in fp32 and in an order fixed by the shape:
    U = proj + (k + the M columns of the set rows, ascending); s = va . tanh(U[:Hd] + q); attn = softmax over all columns;
    t = U[2Hd:] . attn; logits = vp . tanh(U[Hd:2Hd] + t).  Floating inputs of another dtype, layout or device are converted
    through ``.float()`` (autograd sees the cast).  With grad enabled and any floating input requiring grad the call runs
    through a ``torch.autograd.Function`` whose backward is tap_pointer_scores_backward + tap_encode_bits_backward
    (deterministic: no atomics); per step it keeps a clone of ``bits``, ``attn`` (B, nR), ``t`` and ``q`` (B, Hd).  A shape
    without a kernel (``pointer_scores_supported``) raises ValueError."""
    B, _, nR, Hd, rows = _shadow_inputs(bits, "proj", proj, M, rows, lambda B, S, nR, Hd: (
        ("k", k, (3 * Hd,)), ("q", q, (B, Hd)), ("va", va, (Hd,)), ("vp", vp, (Hd,))))
    dev, bits = _bits_on_device(bits)
    args = [_prep_f32(v, dev) for v in (proj, M, k, q, va, vp)]
    if torch.is_grad_enabled() and any(v.requires_grad for v in args):
        return _PointerScores.apply(args[0], bits, *args[1:], rows)
    proj, M, k, q, va, vp = (v.detach() for v in args)
    logits, attn, t = _scores_outputs(B, nR, Hd, dev)
    _scores_into(proj, bits, M, k, q, va, vp, rows, logits, attn, t)
    return logits


def pointer_scores_static_supported(rows, nR, Hd, S):
    """whether tap_pointer_scores_static has a kernel for this shape: ``pointer_scores_supported`` and 1 <= S <= 8 static rows"""
    return 1 <= int(S) <= 8 and pointer_scores_supported(rows, nR, Hd)


def _static_named(G, g, k, q, va, vp, *more):
    """the named shapes of the static-rows forms, for ``_shadow_inputs``; ``more``: (name, tensor) pairs of shape (B, nR)"""
    return lambda B, S, nR, Hd: (("G", G, (3 * Hd, S)), ("g", g, (3 * Hd,)), ("k", k, (3 * Hd,)), ("q", q, (B, Hd)), ("va", va, (Hd,)),
                                 ("vp", vp, (Hd,))) + tuple((nm, v, (B, nR)) for nm, v in more)


def _scores_static_into(xs, bits, G, g, M, k, q, va, vp, rows, logits, attn, t):
    """tap_pointer_scores_static on prepared buffers: one launch on the current stream, nothing allocated"""
    dev = xs.device
    c = _lib.ctx(dev)
    B, S, nR = (int(v) for v in xs.shape)
    Hd = int(q.shape[1])
    _lib.check(_lib.lib().tap_pointer_scores_static(c, _lib.ptr(xs), _lib.ptr(bits), B, nR, rows, Hd, S, _lib.ptr(G), _lib.ptr(g),
                                                    _lib.ptr(M), _lib.ptr(k), _lib.ptr(q), _lib.ptr(va), _lib.ptr(vp),
                                                    _lib.ptr(logits), _lib.ptr(attn), _lib.ptr(t), _lib.stream_of(dev)), c)


class _PointerScoresStatic(torch.autograd.Function):
    """pointer_scores_static under autograd: forward = the one launch, backward = tap_pointer_scores_static_backward (dU,
    dq, dva, dvp), tap_encode_bits_backward on dU (dM and the bias sum, which is dk and dg alike) and dG = sum_b dU[b] xs[b]^T
    as ``_CriticValue.backward`` computes its dG.  What a step keeps beside its parameters: a CLONE of the shadow, attn (B, nR),
    t and q (B, Hd), and ``xs`` by reference; dU is a temporary of the backward and is returned to nobody."""

    @staticmethod
    def forward(ctx, xs, bits, G, g, M, k, q, va, vp, rows):
        B, S, nR = (int(v) for v in xs.shape)
        logits, attn, t = _scores_outputs(B, nR, int(q.shape[1]), xs.device)
        _scores_static_into(xs, bits, G, g, M, k, q, va, vp, rows, logits, attn, t)
        ctx.save_for_backward(xs, bits.clone(), G, g, M, k, q, va, vp, attn, t)
        ctx.rows = rows
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        xs, bits, G, g, *rest = ctx.saved_tensors
        dU, dq, dva, dvp, dM, dk = _pointer_backward(xs, (G, g), bits, *rest, grad, ctx.rows)
        # dG = sum_b dU[b] xs[b]^T: one batched product that reads dU once, then the batch sum of (B, 3 Hd, S); dk[x] = dg[x]
        dG = torch.bmm(dU, xs.transpose(1, 2)).sum(0)
        return None, None, dG, dk, dM, dk.clone(), dq, dva, dvp, None


def pointer_scores_static(xs, bits, G, g, M, k, q, va, vp, rows=None):
    """``pointer_scores`` without ``proj`` (tapenv.h: tap_pointer_scores_static): the static term of U is computed inside the
    launch from the S = 1 .. 8 rows of ``static`` that the static encoder sees -> logits (B, nR) float32.
    ``xs`` (B, S, nR) that slice of ``static``; ``G`` (3 Hd, S) and ``g`` (3 Hd,) the static encoder folded into the two W
    (``tools.Pointer.fold_static`` builds them); the rest as ``pointer_scores`` takes it.  Per env and column, in fp32:
    P = g, then fmaf(G[:, i], xs[i], .) for i ascending; U = P + (k + the M columns of the set rows, ascending); s, attn, t and
    the logits as in ``pointer_scores`` -- with a ``proj`` that equals P bit for bit, the same bytes.  Floating inputs of
    another dtype, layout or device are converted through ``.float()``.  With grad enabled and any parameter requiring grad
    the call runs through a ``torch.autograd.Function`` whose backward is tap_pointer_scores_static_backward +
    tap_encode_bits_backward and one batched product for dG (deterministic: no atomics); per step it keeps a clone of
    ``bits``, ``attn`` (B, nR), ``t`` and ``q`` (B, Hd), and ``xs`` by reference.  ``xs`` and ``bits`` get no gradient.  A
    shape without a kernel (``pointer_scores_static_supported``) raises ValueError."""
    B, S, nR, Hd, rows = _shadow_inputs(bits, "xs", xs, M, rows, _static_named(G, g, k, q, va, vp))
    dev, bits = _bits_on_device(bits)
    xs = _prep_f32(xs.detach(), dev)
    args = [_prep_f32(v, dev) for v in (G, g, M, k, q, va, vp)]
    if torch.is_grad_enabled() and any(v.requires_grad for v in args):
        return _PointerScoresStatic.apply(xs, bits, *args, rows)
    args = [v.detach() for v in args]
    logits, attn, t = _scores_outputs(B, nR, Hd, dev)
    _scores_static_into(xs, bits, *args, rows, logits, attn, t)
    return logits


def pointer_pick_static_supported(rows, nR, Hd, S):
    """whether tap_pointer_pick_static has a kernel for this shape: ``pointer_scores_static_supported``'s shapes"""
    return pointer_scores_static_supported(rows, nR, Hd, S)


def _rows_view_stride(xs):
    """the env stride (in elements) of an ``xs`` (B, S, nR) that the fused launch can read in place -- the last axis
    contiguous, the rows nR apart, the envs at least S nR apart --, else None"""
    B, S, nR = (int(v) for v in xs.shape)
    sb, ss, sc = (int(v) for v in xs.stride())
    if (nR > 1 and sc != 1) or (S > 1 and ss != nR) or (B > 1 and sb < S * nR):
        return None
    return sb if B > 1 else S * nR


def _pick_static_into(xs, stride, bits, G, g, M, k, q, va, vp, mask, rec, rows, ptr, logp, logits):
    """tap_pointer_pick_static on prepared buffers: one launch on the current stream, nothing allocated.  ``rec``: a checked
    PickRecord (DRAW) or None (GREEDY)"""
    dev = xs.device
    c = _lib.ctx(dev)
    B, S, nR = (int(v) for v in xs.shape)
    Hd = int(q.shape[1])
    if rec is None:
        form, state, step, off = _lib.TAP_PICK_GREEDY, None, 0, 0
    else:
        if rec.state.device != dev:
            raise ValueError("the pick's state lives on %s, the step's tensors on %s: the launch reads the state on its own device"
                             % (rec.state.device, dev))
        form, state, step, off = _lib.TAP_PICK_DRAW, rec.state, int(rec.step) & _M32, int(rec.env_offset) & _M32
    _lib.check(_lib.lib().tap_pointer_pick_static(c, _lib.ptr(xs), stride, _lib.ptr(bits), B, nR, rows, Hd, S, _lib.ptr(G), _lib.ptr(g),
                                                  _lib.ptr(M), _lib.ptr(k), _lib.ptr(q), _lib.ptr(va), _lib.ptr(vp), _lib.ptr(mask),
                                                  form, _lib.ptr(state), step, off, _lib.ptr(ptr), _lib.ptr(logp), _lib.ptr(logits),
                                                  _lib.stream_of(dev)), c)


def pointer_pick_static(xs, bits, G, g, M, k, q, va, vp, mask, source=None, rows=None, want_logits=False):
    """``pointer_scores_static`` and the decoding head in ONE launch (tapenv.h: tap_pointer_pick_static), for inference on
    windows whose static rows change every step -> (ptr (B,) int64, logp (B,) float32[, logits (B, nR) float32]).  The logits stay
    in the launch's LDS: no ``attn``, no ``t``, no head launch.  ``xs`` (B, S, nR) may be a view whose last axis is contiguous
    and whose rows are nR apart -- ``static[:, 1:, :]`` of a (B, 1 + S, nR) window is read where it lies, without a copy --;
    anything else is made contiguous.  ``mask`` (B, nR): the stepper's ``current_mask``.  ``source`` None picks greedily
    (``pointer_pick(logits, mask)``'s bytes on ``pointer_scores_static``'s logits); a ``tools.StepDropout`` -- the call takes
    its next pick record --, a ``PickRecord`` or a plain (state, step[, env_offset]) draws (``pointer_pick_draw``'s bytes).
    The other arguments as ``pointer_scores_static`` takes them.  No autograd: with grad enabled, an input that requires grad
    raises ValueError (use ``pointer_scores_static`` and the head).  A shape without a kernel
    (``pointer_pick_static_supported``) raises ValueError."""
    B, S, nR, Hd, rows = _shadow_inputs(bits, "xs", xs, M, rows, _static_named(G, g, k, q, va, vp, ("mask", mask)))
    if torch.is_grad_enabled() and any(v.requires_grad for v in (xs, G, g, M, k, q, va, vp, mask)):
        raise ValueError("pointer_pick_static has no backward: call it under torch.no_grad(), or use pointer_scores_static and "
                         "pointer_pick")
    rec = None if source is None else _pick_record(source)
    dev, bits = _bits_on_device(bits)
    xs = xs.detach()
    stride = _rows_view_stride(xs) if xs.dtype is torch.float32 and xs.device == dev else None
    if stride is None:
        xs = _prep_f32(xs, dev)
        stride = S * nR
    G, g, M, k, q, va, vp, mask = (_prep_f32(v.detach(), dev) for v in (G, g, M, k, q, va, vp, mask))
    ptr = torch.empty(B, dtype=torch.int64, device=dev)
    logp = torch.empty(B, dtype=torch.float32, device=dev)
    logits = torch.empty(B, nR, dtype=torch.float32, device=dev) if want_logits else None
    _pick_static_into(xs, stride, bits, G, g, M, k, q, va, vp, mask, rec, rows, ptr, logp, logits)
    return (ptr, logp, logits) if want_logits else (ptr, logp)


def critic_value_supported(rows, nR, H, S, blocks):
    """whether tap_critic_value has a kernel for this shape: a window with a shadow, H 64, 128 or 256, 1 <= S <= 8 static
    rows and 1 <= blocks <= 8 process blocks"""
    return int(H) in (64, 128, 256) and 1 <= int(S) <= 8 and 1 <= int(blocks) <= 8 and \
        _lib.lib().tap_bits_words(int(rows), int(nR)) > 0


def _critic_into(x, bits, G, g, M, q0, v, w2, b2, blocks, rows, value, z, p, xbar, q):
    """tap_critic_value on prepared buffers: one launch on the current stream, nothing allocated.  q0 (B, H) or (1, H):
    one row serves the whole batch (stride 0)"""
    dev = x.device
    c = _lib.ctx(dev)
    B, S, nR = (int(d) for d in x.shape)
    H = int(M.shape[0])
    stride = 0 if int(q0.shape[0]) == 1 else H
    _lib.check(_lib.lib().tap_critic_value(c, _lib.ptr(x), _lib.ptr(bits), B, nR, rows, H, S, blocks, _lib.ptr(G), _lib.ptr(g),
                                           _lib.ptr(M), _lib.ptr(q0), stride, _lib.ptr(v), _lib.ptr(w2), _lib.ptr(b2),
                                           _lib.ptr(value), _lib.ptr(z), _lib.ptr(p), _lib.ptr(xbar), _lib.ptr(q),
                                           _lib.stream_of(dev)), c)


def _critic_buffers(B, S, nR, H, blocks, dev):
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    return f(B), f(B, H), f(B, blocks, nR), f(B, blocks, S), f(B, blocks, H)


class _CriticValue(torch.autograd.Function):
    """critic_value under autograd: forward = the one launch, backward = tap_critic_value_backward (dU, dq, dv) and
    tap_encode_bits_backward on dU (dM and the shared bias sum); the sums over the batch are torch ops on those tensors.
    What a call keeps beside its parameters: a CLONE of the shadow (the stepper's shadow buffers alternate), ``x`` by
    reference, z (B, H), p (B, n, nR), xbar (B, n, S) and q (B, n, H) -- nothing of size H * nR per env."""

    @staticmethod
    def forward(ctx, x, bits, G, g, M, q0, v, w2, b2, blocks, rows):
        B, S, nR = (int(d) for d in x.shape)
        H = int(M.shape[0])
        value, z, p, xbar, q = _critic_buffers(B, S, nR, H, blocks, x.device)
        _critic_into(x, bits, G, g, M, q0, v, w2, b2, blocks, rows, value, z, p, xbar, q)
        ctx.save_for_backward(x, bits.clone(), G, g, M, v, w2, z, p, xbar, q)
        ctx.dims = (B, S, nR, H, blocks, rows, int(q0.shape[0]))
        return value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gv):
        x, bits, G, g, M, v, w2, z, p, xbar, q = ctx.saved_tensors
        B, S, nR, H, n, rows, q0_rows = ctx.dims
        dev = x.device
        L, P = _lib.lib(), _lib.ptr
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        if B == 0:
            zero = lambda t: torch.zeros_like(t)
            return None, None, zero(G), zero(g), zero(M), f(q0_rows, H).zero_(), zero(v), zero(w2), f(1).zero_(), None, None
        gv = _prep_f32(gv, dev)
        relu = z.clamp_min(0)
        dz = gv.unsqueeze(1) * w2.unsqueeze(0) * (z > 0).to(torch.float32)
        dU, dq, dv, dM, dk = f(B, H, nR), f(B, n, H), f(H), f(H, rows), f(H)
        _backward_on_bits(bits, rows, dU, dM, dk, int(L.tap_critic_value_backward_scratch(B, nR, rows, H, S, n)),
                          lambda c, scratch, need, st: L.tap_critic_value_backward(
                              c, P(x), P(bits), B, nR, rows, H, S, n, P(G), P(g), P(M), P(v), P(q), P(p), P(dz), P(dU), P(dq), P(dv),
                              scratch, need, st))
        dq1 = dq[:, 1:].reshape(-1, H)
        # dG0 = sum_b dU[b] x[b]^T: one batched product that reads dU once, then the batch sum of (B, H, S)
        dG = torch.cat((torch.bmm(dU, x.transpose(1, 2)).sum(0), dq1.t().matmul(xbar[:, :-1].reshape(-1, S)),
                        dz.t().matmul(xbar[:, -1])), 0)
        dg = torch.cat((dk, dq1.sum(0), dz.sum(0)), 0)
        dq0 = dq[:, 0] if q0_rows == B else dq[:, 0].sum(0, keepdim=True)
        return None, None, dG, dg, dM, dq0, dv, gv.matmul(relu), gv.sum().reshape(1), None, None


def critic_value(x, bits, G, g, M, q0, v, w2, b2, blocks, rows=None):
    """The state critic's value estimate on the bit shadow (tapenv.h: tap_critic_value; the reference's realCritic,
    trainer.py:18-94, after its GRU step) in ONE launch -> value (B,) float32.
    ``x`` (B, S, nR) the critic's static input; ``bits`` int64 in ``pack.dynamic_bits`` layout, (B, nR) -- (B, 2 * nR) or
    (B, 2, nR) above 64 rows; ``G`` (3 H, S), ``g`` (3 H,), ``M`` (H, rows) the encoders folded into the attention's W and
    fc.0 (``tools.StateCritic.fold`` builds them); ``q0`` (B, H), or (1, H) / (H,) for one row that serves the whole batch;
    ``v`` / ``w2`` (H,); ``b2`` (1,) or a scalar tensor; ``blocks`` the number of process blocks.  ``rows`` defaults to
    ``M.shape[1]``; bits at positions >= rows are ignored.  Per env, in fp32 and in an order fixed by the shape:
    U = g[:H] + the M columns of the set rows (ascending) + G[:H] . x; per block s = v . tanh(U + q), p = softmax over all
    columns, xbar = x . p, q = g[H:2H] + G[H:2H] . xbar; z = g[2H:] + G[2H:] . xbar; value = b2 + w2 . relu(z).
    Floating inputs of another dtype, layout or device are converted through ``.float()`` (autograd sees the cast).  With
    grad enabled and any parameter requiring grad the call runs through a ``torch.autograd.Function`` whose backward is
    tap_critic_value_backward + tap_encode_bits_backward (deterministic: no atomics); it keeps a clone of ``bits``, ``x``
    by reference, and z (B, H), p (B, blocks, nR), xbar (B, blocks, S), q (B, blocks, H).  ``x`` and ``bits`` get no
    gradient.  A shape without a kernel (``critic_value_supported``) raises ValueError."""
    blocks = int(blocks)
    if q0.dim() == 1:
        q0 = q0.unsqueeze(0)
    if b2.dim() == 0:
        b2 = b2.reshape(1)
    B, S, nR, H, rows = _shadow_inputs(bits, "x", x, M, rows, lambda B, S, nR, H: (
        ("G", G, (3 * H, S)), ("g", g, (3 * H,)), ("q0", q0, (B, H), (1, H)), ("v", v, (H,)), ("w2", w2, (H,)), ("b2", b2, (1,))),
        blocks)
    dev, bits = _bits_on_device(bits)
    x = _prep_f32(x.detach(), dev)
    args = [_prep_f32(t, dev) for t in (G, g, M, q0, v, w2, b2)]
    if torch.is_grad_enabled() and any(t.requires_grad for t in args):
        return _CriticValue.apply(x, bits, *args, blocks, rows)
    args = [t.detach() for t in args]
    value, z, p, xbar, q = _critic_buffers(B, S, nR, H, blocks, dev)
    _critic_into(x, bits, *args, blocks, rows, value, z, p, xbar, q)
    return value


def decoder_step_supported(Ks, Kd, Hd):
    """whether tap_decoder_step has a kernel for this shape: Hd 64, 128 or 256 and 1 <= Ks + Kd <= Hd + 16"""
    Ks, Kd, Hd = int(Ks), int(Kd), int(Hd)
    return Hd in (64, 128, 256) and Ks >= 0 and Kd >= 0 and 1 <= Ks + Kd <= Hd + 16


def _decoder_into(xs, xd, h, P, c, w_hh, b_hh, wq, h_out, q_out, gates):
    """tap_decoder_step on prepared buffers (xs / xd (B, Ks) / (B, Kd) or None, h (B, Hd) or None, gates (B, 4, Hd) or
    None): one launch on the current stream, nothing allocated"""
    dev = P.device
    c_ = _lib.ctx(dev)
    B, Hd = int(h_out.shape[0]), int(h_out.shape[1])
    Ks = 0 if xs is None else int(xs.shape[1])
    Kd = 0 if xd is None else int(xd.shape[1])
    _lib.check(_lib.lib().tap_decoder_step(c_, _lib.ptr(xs), Ks, _lib.ptr(xd), Kd, _lib.ptr(h), B, Hd, _lib.ptr(P), _lib.ptr(c),
                                           _lib.ptr(w_hh), _lib.ptr(b_hh), _lib.ptr(wq), _lib.ptr(h_out), _lib.ptr(q_out),
                                           _lib.ptr(gates), _lib.stream_of(dev)), c_)


def _decoder_backward_into(gates, h, g, dgi, dghn, carry):
    """tap_decoder_step_backward on prepared buffers: one launch on the current stream, nothing allocated"""
    dev = gates.device
    c_ = _lib.ctx(dev)
    B, Hd = int(g.shape[0]), int(g.shape[1])
    _lib.check(_lib.lib().tap_decoder_step_backward(c_, B, Hd, _lib.ptr(gates), _lib.ptr(h), _lib.ptr(g), _lib.ptr(dgi),
                                                    _lib.ptr(dghn), _lib.ptr(carry), _lib.stream_of(dev)), c_)


# ---- dropout inside the decoder step's launch (tapenv.h: tap_decoder_step_dropout has the definition) -------------------
_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_M32 = 0xFFFFFFFF

StepDropoutRecord = collections.namedtuple("StepDropoutRecord", "state step p_rnn p_hh env_offset")
StepDropoutRecord.__doc__ = """what a dropout step takes: ``state`` the int64[2] (seed, episode) tensor, ``step`` the decoding step
(a Python int), the two probabilities and the index of the call's first env in the whole batch (``tools.StepDropout.take_step``)"""


def dropout_threshold(p):
    """keep iff word >= min(2^32 - 1, round(p 2^32))"""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("a dropout probability lies in [0, 1], got %r" % (p,))
    return min(_M32, int(math.floor(p * 4294967296.0 + 0.5)))


def dropout_scale(p):
    """what a kept element is multiplied by: float32(1 / (1 - p)), as a Python float"""
    return struct.unpack("f", struct.pack("f", 1.0 / (1.0 - float(p))))[0]


def _mulhilo32(m, c):
    """the 64-bit product of the constant m < 2^32 and an int64 tensor of values < 2^32 -> (high, low) 32-bit halves, in
    int64 arithmetic that never passes 2^49"""
    lo16 = m * (c & 0xFFFF)
    t = m * (c >> 16) + (lo16 >> 16)
    return t >> 16, ((t & 0xFFFF) << 16) | (lo16 & 0xFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 in torch integer ops: ``counter`` four and ``key`` two int64 tensors (or ints) of values < 2^32, which
    broadcast -> the four output words, int64 tensors of values < 2^32"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        hi0, lo0 = _mulhilo32(_PHILOX_M[0], c0)
        hi1, lo1 = _mulhilo32(_PHILOX_M[1], c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _PHILOX_W[0]) & _M32, (k1 + _PHILOX_W[1]) & _M32
    return c0, c1, c2, c3


def dropout_keep_words(state, step, B, Hd, p_rnn, p_hh, env_offset=0):
    """The two dropout masks of a decoding step, packed as the kernels write them: (B, 2, Hd / 64) int64 on ``state``'s
    device, plane 0 drop_rnn, plane 1 drop_hh, bit j mod 64 of word j / 64 set iff hidden row j is kept.  ``state`` is the
    int64[2] (seed, episode).  For env b and row j the Philox4x32-10 counter is (env_offset + b, j, step, episode mod 2^32)
    and the key (seed mod 2^32, seed >> 32); output word 0 decides drop_rnn and word 1 drop_hh: keep iff word >=
    ``dropout_threshold(p)``.  Torch integer ops only -- it runs on the CPU, and on the GPU it reads no value on the host,
    so it can be captured in a graph with the ``state`` update in front of it."""
    B, Hd = int(B), int(Hd)
    if Hd < 64 or Hd % 64:
        raise ValueError("the packed masks need Hd to be a multiple of 64, got %d" % Hd)
    if state.dtype is not torch.int64 or tuple(state.shape) != (2,):
        raise ValueError("state must be an int64[2] (seed, episode) tensor, got %s %s" % (state.dtype, tuple(state.shape)))
    dev = state.device
    seed, episode = state[0], state[1]
    env = ((torch.arange(B, dtype=torch.int64, device=dev) + int(env_offset)) & _M32).view(B, 1)
    row = torch.arange(Hd, dtype=torch.int64, device=dev).view(1, Hd)
    zero = torch.zeros(B, Hd, dtype=torch.int64, device=dev)
    w = philox4x32_10((env + zero, row + zero, zero + (int(step) & _M32), zero + (episode & _M32)), (seed & _M32, (seed >> 32) & _M32))
    keep = torch.stack((w[0] >= dropout_threshold(p_rnn), w[1] >= dropout_threshold(p_hh)), dim=1)        # (B, 2, Hd)
    bit = torch.arange(64, dtype=torch.int64, device=dev)
    return (keep.view(B, 2, Hd // 64, 64).to(torch.int64) << bit).sum(-1)


def dropout_keep_mask(words):
    """packed keep words (B, 2, Hd / 64) -> bool (B, 2, Hd)"""
    bit = torch.arange(64, dtype=torch.int64, device=words.device)
    return ((words.unsqueeze(-1) >> bit) & 1).bool().view(int(words.shape[0]), 2, -1)


def _dropout_record(dropout):
    """-> a checked StepDropoutRecord from the record or a plain (state, step, p_rnn, p_hh[, env_offset]) tuple"""
    d = StepDropoutRecord(*dropout) if len(dropout) == 5 else StepDropoutRecord(*dropout, 0)
    if not torch.is_tensor(d.state) or d.state.dtype is not torch.int64 or tuple(d.state.shape) != (2,) or not d.state.is_contiguous():
        raise ValueError("dropout state must be a contiguous int64[2] (seed, episode) tensor")
    for p in (d.p_rnn, d.p_hh):
        if not 0.0 <= float(p) < 1.0:
            raise ValueError("the dropout launch takes 0 <= p < 1, got %r (p = 1 stays on the torch path)" % (p,))
    if int(d.step) < 0 or int(d.env_offset) < 0:
        raise ValueError("dropout step and env_offset must not be negative, got %r and %r" % (d.step, d.env_offset))
    if not d.state.is_cuda:
        raise ValueError("dropout state lives on %s: the launch reads it on the device (tools.StepDropout(seed, device))" % (d.state.device,))
    return d


def _dropout_state_on(drop, dev):
    """the launch dereferences ``state``: it must live on the launch's own device.  It is refused, not copied -- a copy would
    cut a captured graph off from the tensor that ``next_episode()`` advances"""
    if drop.state.device != dev:
        raise ValueError("dropout state lives on %s, the step's tensors on %s: the launch reads the state on its own device"
                         % (drop.state.device, dev))
    return drop


def _drop_scalars(d):
    """the launch arguments of a record: step, env_offset, the two thresholds, the two scales"""
    return (int(d.step) & _M32, int(d.env_offset) & _M32, dropout_threshold(d.p_rnn), dropout_threshold(d.p_hh),
            dropout_scale(d.p_rnn), dropout_scale(d.p_hh))


def _decoder_dropout_into(xs, xd, h, P, c, w_hh, b_hh, wq, drop, h_out, q_out, gates, rnn_out, keep):
    """tap_decoder_step_dropout on prepared buffers (as _decoder_into; ``drop`` a StepDropoutRecord whose state lives on the
    device, rnn_out (B, Hd) or None, keep (B, 2, Hd / 64) int64): one launch on the current stream, nothing allocated"""
    dev = P.device
    _dropout_state_on(drop, dev)
    c_ = _lib.ctx(dev)
    B, Hd = int(h_out.shape[0]), int(h_out.shape[1])
    Ks = 0 if xs is None else int(xs.shape[1])
    Kd = 0 if xd is None else int(xd.shape[1])
    p = _lib.ptr
    _lib.check(_lib.lib().tap_decoder_step_dropout(c_, p(xs), Ks, p(xd), Kd, p(h), B, Hd, p(P), p(c), p(w_hh), p(b_hh), p(wq),
                                                   p(drop.state), *_drop_scalars(drop), p(h_out), p(q_out), p(gates), p(rnn_out),
                                                   p(keep), _lib.stream_of(dev)), c_)


def _decoder_dropout_backward_into(gates, h, g_h, g_r, keep, s_rnn, s_hh, dgi, dghn, carry):
    """tap_decoder_step_dropout_backward on prepared buffers: one launch on the current stream, nothing allocated"""
    dev = gates.device
    c_ = _lib.ctx(dev)
    B, Hd = int(g_h.shape[0]), int(g_h.shape[1])
    p = _lib.ptr
    _lib.check(_lib.lib().tap_decoder_step_dropout_backward(c_, B, Hd, p(gates), p(h), p(g_h), p(g_r), p(keep), s_rnn, s_hh, p(dgi),
                                                            p(dghn), p(carry), _lib.stream_of(dev)), c_)


def _step_outputs(B, Hd, dev, drop, grad):
    """what a step's launch writes -> h_new, q, gates, rnn_out, keep: ``gates`` only for a backward (``grad``), ``rnn_out`` only
    for the backward of a dropout step, the keep words for every dropout step (its launch always writes them) -- the plain
    forms allocate neither"""
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    return (f(B, Hd), f(B, Hd), f(B, 4, Hd) if grad else None, f(B, Hd) if grad and drop is not None else None,
            None if drop is None else torch.empty(B, 2, Hd // 64, dtype=torch.int64, device=dev))


def _step_no_grad(launch, args, drop, B, Hd, dev):
    """a step outside autograd: ``launch`` (_decoder_launch or _decoder_hm_launch) on the detached ``args``, nothing kept"""
    h_new, q, _, _, keep = _step_outputs(B, Hd, dev, drop, False)
    launch([None if v is None else v.detach() for v in args], drop, h_new, q, None, None, keep)
    return h_new, q


def _step_backward_launch(gates, h, g_h, g_q, wq, keep, scales):
    """the element-wise part of a step's backward -> g_q (float32), dgi, dgh, carry.  ``keep`` None, the plain step: q = h' .
    wq^T, so wq^T . dq joins the gradient arriving at h' here, g = g_h + g_q . wq.  A dropout step: the two masks join g_h
    and g_r = g_q . wq at h' inside the launch."""
    B, Hd = int(gates.shape[0]), int(gates.shape[2])
    dev = gates.device
    g_q = _prep_f32(g_q, dev)
    dgi = torch.empty(B, 3 * Hd, dtype=torch.float32, device=dev)
    dghn = torch.empty(B, Hd, dtype=torch.float32, device=dev)
    carry = torch.empty(B, Hd, dtype=torch.float32, device=dev)
    if keep is None:
        _decoder_backward_into(gates, h, _prep_f32(g_h, dev) + g_q.matmul(wq), dgi, dghn, carry)
    else:
        _decoder_dropout_backward_into(gates, h, _prep_f32(g_h, dev), g_q.matmul(wq), keep, scales[0], scales[1], dgi, dghn, carry)
    return g_q, dgi, torch.cat((dgi[:, :2 * Hd], dghn), dim=1), carry            # the r and z parts of dgh are those of dgi


def _step_grads(need, xs, xd, h, hq, P, w_hh, g_q, dgi, dgh, carry):
    """the sums over the batch of a step's backward, as matmuls -> dxs, dxd, dh, dP, dc, dw_hh, db_hh, dwq (None where ``need``,
    eight flags in that order, does not ask).  ``xd`` is the dynamic half of the GRU's input -- the height-map step's enc --,
    ``hq`` what q was formed from: h', or drop_rnn(h') of a dropout step."""
    Ks = 0 if xs is None else int(xs.shape[1])
    x = xd if xs is None else xs if xd is None else torch.cat((xs, xd), dim=1)
    dxs = dgi.matmul(P[:, :Ks]) if xs is not None and need[0] else None
    dxd = dgi.matmul(P[:, Ks:]) if xd is not None and need[1] else None
    dh = carry + dgh.matmul(w_hh) if h is not None and need[2] else None
    dP = dgi.t().matmul(x) if need[3] else None
    dc = dgi.sum(0) if need[4] else None
    dw_hh = (torch.zeros_like(w_hh) if h is None else dgh.t().matmul(h)) if need[5] else None
    db_hh = dgh.sum(0) if need[6] else None
    dwq = g_q.t().matmul(hq) if need[7] else None
    return dxs, dxd, dh, dP, dc, dw_hh, db_hh, dwq


def _drop_scales(drop):
    return None if drop is None else (dropout_scale(drop.p_rnn), dropout_scale(drop.p_hh))


def _decoder_launch(args, drop, h_new, q, gates, rnn_out, keep):
    """the plain or the dropout launch of a step on prepared ``args`` = xs, xd, h, P, c, w_hh, b_hh, wq"""
    if drop is None:
        _decoder_into(*args, h_new, q, gates)
    else:
        _decoder_dropout_into(*args, drop, h_new, q, gates, rnn_out, keep)


class _DecoderStep(torch.autograd.Function):
    """decoder_step and decoder_step_dropout under autograd (``drop`` None or the checked record): forward = the one launch
    with the gates kept, backward = tap_decoder_step_backward (element-wise) and the sums over the batch as matmuls.  What a
    step keeps: xs, xd and h BY REFERENCE (a stepper hands out private copies of its decoder buffers while grad is enabled,
    and h is the previous step's own output), h', and gates (B, 4, Hd) = r, z, n, gh_n; the parameters by reference.
    A dropout step keeps rnn_out = drop_rnn(h') in h''s place (dwq = g_q^T . rnn_out) and the keep words; its backward is
    tap_decoder_step_dropout_backward.  The state tensor is NOT kept -- the masks are, so advancing the episode cannot change
    a pending backward."""

    @staticmethod
    def forward(ctx, xs, xd, h, P, c, w_hh, b_hh, wq, drop):
        B = int((xs if xs is not None else xd).shape[0])
        h_new, q, gates, rnn_out, keep = _step_outputs(B, int(wq.shape[0]), P.device, drop, True)
        _decoder_launch((xs, xd, h, P, c, w_hh, b_hh, wq), drop, h_new, q, gates, rnn_out, keep)
        ctx.save_for_backward(xs, xd, h, h_new if drop is None else rnn_out, gates, P, w_hh, wq, keep)
        ctx.scales = _drop_scales(drop)
        return h_new, q

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_h, g_q):
        xs, xd, h, hq, gates, P, w_hh, wq, keep = ctx.saved_tensors
        g_q, dgi, dgh, carry = _step_backward_launch(gates, h, g_h, g_q, wq, keep, ctx.scales)
        return _step_grads(ctx.needs_input_grad, xs, xd, h, hq, P, w_hh, g_q, dgi, dgh, carry) + (None,)


def decoder_step_dropout(xs, xd, h, P, c, w_hh, b_hh, wq, dropout):
    """``decoder_step`` with the pointer's two dropouts (model.py:112-115) inside the same launch (tapenv.h:
    tap_decoder_step_dropout) -> (drop_hh(h'), wq . drop_rnn(h')).  ``dropout`` = (state, step, p_rnn, p_hh, env_offset) -- a
    ``StepDropoutRecord``, what ``tools.StepDropout.take_step`` hands out: the masks are ``dropout_keep_words`` for that
    record, a kept element is scaled by float32(1 / (1 - p)), a dropped one is +0.0; 0 <= p < 1.  ``state`` is read on the
    device: no host value, capturable, new masks on every replay that advances it.  Under autograd the backward is again
    one element-wise launch (tap_decoder_step_dropout_backward) plus ``decoder_step``'s matmuls; per step it keeps, beside
    ``gates``, drop_rnn(h') and the packed keep words (64 bytes per env at Hd = 256) -- not ``state``, so a later
    ``next_episode()`` cannot change a pending backward.  Everything else as ``decoder_step``, whose signature stays the
    reference-facing one."""
    return _decoder_step(xs, xd, h, P, c, w_hh, b_hh, wq, dropout)


def decoder_step(xs, xd, h, P, c, w_hh, b_hh, wq):
    """The decoder side of a decoding step (tapenv.h: tap_decoder_step; model.py:347-354, the GRU step of 108-115 and the
    decoder's columns of the attention) in ONE launch -> (h_new (B, Hd), q (B, Hd)) float32: the decoder's 1x1 encoders
    folded into the GRU's input weights (``P`` (3 Hd, Ks + Kd), ``c`` (3 Hd,): ``tools.Pointer.fold_decoder``), the GRU cell
    (``w_hh`` (3 Hd, Hd), ``b_hh`` (3 Hd,): weight_hh_l0 / bias_hh_l0, gates r, z, n) and q = wq . h' (``wq`` (Hd, Hd)), what
    ``pointer_scores`` takes.  ``xs`` (B, Ks[, 1]) the chosen block's sides and ``xd`` (B, ...) the container feature, flattened
    to (B, Kd) -- a stepper's ``decoder_static`` / ``decoder_dynamic``, read as two buffers: no concatenation --; either may be
    None (a single encoder).  ``h`` (B, Hd) the previous hidden state, or None for the zero state of step 0.  fp32, every sum
    one chain of fmaf in ascending term order (static columns first): the same bytes on every call.  Floating inputs of
    another dtype, layout or device are converted through ``.float()`` (autograd sees the cast).  With grad enabled and any
    input requiring grad the call runs through a ``torch.autograd.Function``: the backward is one element-wise launch
    (tap_decoder_step_backward) and torch matmuls for the sums over the batch; per step it keeps ``gates`` (B, 4, Hd) and
    h', and ``xs`` / ``xd`` / ``h`` by reference, so the caller must not overwrite them before ``backward()`` (a stepper's
    grad-mode attributes are private copies).  A shape without a kernel (``decoder_step_supported``) raises ValueError.
    ``decoder_step_dropout`` is the training form with the pointer's dropouts inside the launch."""
    return _decoder_step(xs, xd, h, P, c, w_hh, b_hh, wq, None)


def _check_step_params(P, dyn, Ks, Kd, h, B, c, w_hh, b_hh, wq):
    """what both steps check of the GRU's own tensors -> Hd.  ``dyn`` = what the messages call the dynamic half of the input
    and its ``Kd`` values per env: ("xd", "Kd") or ("the encoder", "m")"""
    if P.dim() != 2 or int(P.shape[0]) % 3 or not P.is_floating_point():
        raise ValueError("P must be a floating (3 Hd, Ks + %s) tensor, got %s %s" % (dyn[1], P.dtype, tuple(P.shape)))
    Hd = int(P.shape[0]) // 3
    if Ks + Kd != int(P.shape[1]):
        raise ValueError("P has %d columns, xs and %s have %d + %d values per env" % (int(P.shape[1]), dyn[0], Ks, Kd))
    for name, v, shape in (("c", c, (3 * Hd,)), ("w_hh", w_hh, (3 * Hd, Hd)), ("b_hh", b_hh, (3 * Hd,)), ("wq", wq, (Hd, Hd))) + \
            ((("h", h, (B, Hd)),) if h is not None else ()):
        if tuple(v.shape) != shape or not v.is_floating_point():
            raise ValueError("%s must be a floating %s tensor, got %s %s" % (name, shape, v.dtype, tuple(v.shape)))
    return Hd


def _step_record_on(dropout, P):
    """-> (the checked record or None, the step's device); a record whose state lives on another device is refused"""
    drop = None if dropout is None else _dropout_record(dropout)
    dev = _lib.resolve_device(P.device)
    if drop is not None:
        _dropout_state_on(drop, dev)
    return drop, dev


def _decoder_step(xs, xd, h, P, c, w_hh, b_hh, wq, dropout):
    if xs is None and xd is None:
        raise ValueError("decoder_step needs xs, xd or both")
    B = int((xs if xs is not None else xd).shape[0])
    for name, v in (("xs", xs), ("xd", xd)):
        if v is not None and (v.dim() < 2 or int(v.shape[0]) != B or not v.is_floating_point()):
            raise ValueError("%s must be a floating (%d, ...) tensor, got %s %s" % (name, B, v.dtype, tuple(v.shape)))
    xs = None if xs is None else xs.reshape(B, -1)
    xd = None if xd is None else xd.reshape(B, -1)
    Ks, Kd = (0 if v is None else int(v.shape[1]) for v in (xs, xd))
    xs, xd = (None if v is None or int(v.shape[1]) == 0 else v for v in (xs, xd))
    Hd = _check_step_params(P, ("xd", "Kd"), Ks, Kd, h, B, c, w_hh, b_hh, wq)
    if not decoder_step_supported(Ks, Kd, Hd):
        raise ValueError("no decoder-step kernel for Ks %d, Kd %d, Hd %d (Hd 64 / 128 / 256, 1 <= Ks + Kd <= Hd + 16)" % (Ks, Kd, Hd))
    drop, dev = _step_record_on(dropout, P)
    args = [_prep_f32(v, dev) for v in (xs, xd, h, P, c, w_hh, b_hh, wq)]
    if torch.is_grad_enabled() and any(v is not None and v.requires_grad for v in args):
        return _DecoderStep.apply(*args, drop)
    return _step_no_grad(_decoder_launch, args, drop, B, Hd, dev)


def decoder_step_heightmap_supported(Ks, C, W, L, m, Hd):
    """whether tap_decoder_step_hm has a kernel for this shape: Hd 64, 128 or 256, m = Hd / 2 or Hd, C 1, 2 or 4,
    1 <= W, L <= 12, 0 <= Ks <= 16 and Ks + m <= Hd + 16"""
    Ks, C, W, L, m, Hd = int(Ks), int(C), int(W), int(L), int(m), int(Hd)
    return Hd in (64, 128, 256) and m in (Hd // 2, Hd) and C in (1, 2, 4) and 1 <= W <= 12 and 1 <= L <= 12 and \
        0 <= Ks <= 16 and Ks + m <= Hd + 16


def _decoder_hm_into(xs, hm, h, enc_w, P, c, w_hh, b_hh, wq, h_out, q_out, gates, enc_out):
    """tap_decoder_step_hm on prepared buffers (xs (B, Ks) or None, hm (B, C, W, L), h (B, Hd) or None, enc_w = (w1, b1, w2,
    b2, w3, b3) with w3's leading axis m, gates (B, 4, Hd) or None, enc_out (B, m) or None): one launch on the current
    stream, nothing allocated"""
    dev = P.device
    c_ = _lib.ctx(dev)
    B, Hd = int(h_out.shape[0]), int(h_out.shape[1])
    Ks = 0 if xs is None else int(xs.shape[1])
    C, W, L = (int(v) for v in hm.shape[1:])
    p = _lib.ptr
    _lib.check(_lib.lib().tap_decoder_step_hm(c_, p(xs), Ks, p(hm), C, W, L, p(h), B, Hd, int(enc_w[4].shape[0]), *(p(w) for w in enc_w),
                                              p(P), p(c), p(w_hh), p(b_hh), p(wq), p(h_out), p(q_out), p(gates), p(enc_out),
                                              _lib.stream_of(dev)), c_)


def _leaky_slope(z):
    return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.01))


def _decoder_hm_dropout_into(xs, hm, h, enc_w, P, c, w_hh, b_hh, wq, drop, h_out, q_out, gates, enc_out, rnn_out, keep):
    """tap_decoder_step_hm_dropout on prepared buffers (as _decoder_hm_into and _decoder_dropout_into): one launch on the
    current stream, nothing allocated"""
    dev = P.device
    _dropout_state_on(drop, dev)
    c_ = _lib.ctx(dev)
    B, Hd = int(h_out.shape[0]), int(h_out.shape[1])
    Ks = 0 if xs is None else int(xs.shape[1])
    C, W, L = (int(v) for v in hm.shape[1:])
    p = _lib.ptr
    _lib.check(_lib.lib().tap_decoder_step_hm_dropout(c_, p(xs), Ks, p(hm), C, W, L, p(h), B, Hd, int(enc_w[4].shape[0]),
                                                      *(p(w) for w in enc_w), p(P), p(c), p(w_hh), p(b_hh), p(wq), p(drop.state),
                                                      *_drop_scalars(drop), p(h_out), p(q_out), p(gates), p(enc_out), p(rnn_out),
                                                      p(keep), _lib.stream_of(dev)), c_)


def _decoder_hm_launch(args, drop, h_new, q, gates, rnn_out, keep, enc=None):
    """_decoder_launch for the height-map step: ``args`` = xs, hm, h, the encoder's six tensors, P, c, w_hh, b_hh, wq"""
    xs, hm, h = args[:3]
    if drop is None:
        _decoder_hm_into(xs, hm, h, tuple(args[3:9]), *args[9:], h_new, q, gates, enc)
    else:
        _decoder_hm_dropout_into(xs, hm, h, tuple(args[3:9]), *args[9:], drop, h_new, q, gates, enc, rnn_out, keep)


class _DecoderStepHeightmap(torch.autograd.Function):
    """decoder_step_heightmap and decoder_step_heightmap_dropout under autograd (``drop`` None or the checked record): forward
    = the one launch with gates and enc kept; backward = _DecoderStep's (the element-wise launch and the matmuls over the
    batch, with xd = enc), then the encoder's six gradients and hm's from d_enc by recomputing a1 / a2 in torch on the
    gathered cells hm[:, :, ::4, ::4].  Inputs by reference, and rnn_out and the keep words of a dropout step, as
    _DecoderStep; the encoder's backward is the same for both: it receives d_enc."""

    @staticmethod
    def forward(ctx, xs, hm, h, w1, b1, w2, b2, w3, b3, P, c, w_hh, b_hh, wq, drop):
        B, dev = int(hm.shape[0]), P.device
        h_new, q, gates, rnn_out, keep = _step_outputs(B, int(wq.shape[0]), dev, drop, True)
        enc = torch.empty(B, int(w3.shape[0]), dtype=torch.float32, device=dev)
        _decoder_hm_launch((xs, hm, h, w1, b1, w2, b2, w3, b3, P, c, w_hh, b_hh, wq), drop, h_new, q, gates, rnn_out, keep, enc)
        ctx.save_for_backward(xs, hm, h, h_new if drop is None else rnn_out, gates, enc, w1, b1, w2, b2, w3, P, w_hh, wq, keep)
        ctx.scales = _drop_scales(drop)
        return h_new, q

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_h, g_q):
        xs, hm, h, hq, gates, enc, w1, b1, w2, b2, w3, P, w_hh, wq, keep = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_q, dgi, dgh, carry = _step_backward_launch(gates, h, g_h, g_q, wq, keep, ctx.scales)
        dxs, d_enc, dh, dP, dc, dw_hh, db_hh, dwq = _step_grads((need[0], need[1] or any(need[3:9]), need[2]) + tuple(need[9:14]),
                                                               xs, enc, h, hq, P, w_hh, g_q, dgi, dgh, carry)
        dhm, dw1, db1, dw2, db2, dw3, db3 = _heightmap_encoder_backward(need, d_enc, hm, w1, b1, w2, b2, w3)
        return dxs, dhm, dh, dw1, db1, dw2, db2, dw3, db3, dP, dc, dw_hh, db_hh, dwq, None


def _heightmap_encoder_backward(need, d_enc, hm, w1, b1, w2, b2, w3):
    """the encoder's half of a height-map step's backward, from d_enc = dgi . P[:, Ks:] (B, m), or None when nothing of the
    encoder asks: the two hidden layers recomputed in torch on the gathered cells -> dhm, dw1, db1, dw2, db2, dw3, db3 (None
    where ``need``, the Function's needs_input_grad, does not ask)"""
    dhm = dw1 = db1 = dw2 = db2 = dw3 = db3 = None
    if d_enc is not None:
        B = int(hm.shape[0])
        cells = hm[:, :, ::4, ::4]                                # (B, C, nw, nl)
        C, nw, nl = (int(v) for v in cells.shape[1:])
        Np, C1, C2 = nw * nl, int(w1.shape[0]), int(w2.shape[0])
        cells = cells.reshape(B, C, Np).transpose(1, 2)           # (B, Np, C)
        z1 = cells.matmul(w1.t()) + b1
        a1 = z1 * _leaky_slope(z1)                                # (B, Np, C1)
        z2 = a1.matmul(w2.t()) + b2
        a2 = z2 * _leaky_slope(z2)                                # (B, Np, C2); conv3 reads it as t = c2 Np + p
        dw3 = d_enc.t().matmul(a2.transpose(1, 2).reshape(B, C2 * Np)) if need[7] else None
        db3 = d_enc.sum(0) if need[8] else None
        dz2 = d_enc.matmul(w3).view(B, C2, Np).transpose(1, 2) * _leaky_slope(z2)
        dw2 = dz2.reshape(B * Np, C2).t().matmul(a1.reshape(B * Np, C1)) if need[5] else None
        db2 = dz2.sum((0, 1)) if need[6] else None
        dz1 = dz2.matmul(w2) * _leaky_slope(z1)
        dw1 = dz1.reshape(B * Np, C1).t().matmul(cells.reshape(B * Np, C)) if need[3] else None
        db1 = dz1.sum((0, 1)) if need[4] else None
        if need[1]:
            dhm = torch.zeros_like(hm)
            dhm[:, :, ::4, ::4] = dz1.matmul(w1).transpose(1, 2).reshape(B, C, nw, nl)
    return dhm, dw1, db1, dw2, db2, dw3, db3


def decoder_step_heightmap_dropout(xs, hm, h, encoder, P, c, w_hh, b_hh, wq, dropout):
    """``decoder_step_heightmap`` with the pointer's two dropouts inside the same launch (tapenv.h:
    tap_decoder_step_hm_dropout) -> (drop_hh(h'), wq . drop_rnn(h')); ``dropout`` and what a step keeps as
    ``decoder_step_dropout``.  The encoder stage and its backward are untouched: the backward receives d_enc as before."""
    return _decoder_step_heightmap(xs, hm, h, encoder, P, c, w_hh, b_hh, wq, dropout)


def decoder_step_heightmap(xs, hm, h, encoder, P, c, w_hh, b_hh, wq):
    """``decoder_step`` for a 3D actor, still ONE launch (tapenv.h: tap_decoder_step_hm) -> (h_new (B, Hd), q (B, Hd)) float32:
    the reference's ``HeightmapEncoder`` (model.py:21-35; two leaky-ReLUs, so it does not fold) runs on the tile of envs in
    front of the input product, which takes its dynamic terms enc (B, m) from the LDS.  ``xs`` (B, Ks[, 1]) the chosen
    block's sides, or None; ``hm`` (B, C, W, L) the stepper's ``decoder_dynamic``; ``h`` (B, Hd) or None for the zero state;
    ``encoder`` a ``tools.HeightmapEncoder`` or anything with ``conv1`` (m / 4, C, 1, 1), ``conv2`` (m / 2, m / 4, 1, 1) and
    ``conv3`` (m, m / 2, ceil(W / 4), ceil(L / 4)), all with a bias; ``P`` (3 Hd, Ks + m) and ``c`` from
    ``tools.Pointer.fold_decoder(static, encoder)`` (m identity columns for the dynamic half); the rest as ``decoder_step``.
    fp32, every sum one chain of fmaf in ascending order, the encoder's from their biases: the same bytes on every call.
    With grad enabled and any input requiring grad the call runs through a ``torch.autograd.Function``: the backward reuses
    tap_decoder_step_backward and ``decoder_step``'s matmuls, and gets the encoder's six parameter gradients -- and ``hm``'s,
    scattered back to the cells (4i, 4j) -- from d_enc by recomputing the two hidden layers in torch; per step it keeps
    ``gates``, h' and enc, and the inputs by reference.  A shape without a kernel
    (``decoder_step_heightmap_supported``) raises ValueError.  ``decoder_step_heightmap_dropout`` is the training form."""
    return _decoder_step_heightmap(xs, hm, h, encoder, P, c, w_hh, b_hh, wq, None)


def _decoder_step_heightmap(xs, hm, h, encoder, P, c, w_hh, b_hh, wq, dropout):
    if hm is None or hm.dim() != 4 or not hm.is_floating_point():
        raise ValueError("hm must be a floating (B, C, W, L) tensor, got %s" % (None if hm is None else "%s %s" % (hm.dtype, tuple(hm.shape)),))
    B, C, W, L = (int(v) for v in hm.shape)
    if xs is not None and (xs.dim() < 2 or int(xs.shape[0]) != B or not xs.is_floating_point()):
        raise ValueError("xs must be a floating (%d, ...) tensor, got %s %s" % (B, xs.dtype, tuple(xs.shape)))
    xs = None if xs is None else xs.reshape(B, -1)
    Ks = 0 if xs is None else int(xs.shape[1])
    xs = xs if Ks else None
    convs = [getattr(encoder, name, None) for name in ("conv1", "conv2", "conv3")]
    if any(cv is None or getattr(cv, "weight", None) is None or cv.weight.dim() != 4 or getattr(cv, "bias", None) is None for cv in convs):
        raise ValueError("encoder must have conv1, conv2 and conv3 with four-axis weights and biases (tools.HeightmapEncoder)")
    m = int(convs[2].weight.shape[0])
    nw, nl = (W + 3) // 4, (L + 3) // 4
    shapes = ((m // 4, C, 1, 1), (m // 2, m // 4, 1, 1), (m, m // 2, nw, nl))
    for name, cv, shape in zip(("conv1", "conv2", "conv3"), convs, shapes):
        if m % 4 or tuple(cv.weight.shape) != shape or tuple(cv.bias.shape) != shape[:1] or not cv.weight.is_floating_point():
            raise ValueError("encoder.%s must be a floating %s convolution for a %s map and hidden size %d, got %s"
                             % (name, shape, (C, W, L), m, tuple(cv.weight.shape)))
    Hd = _check_step_params(P, ("the encoder", "m"), Ks, m, h, B, c, w_hh, b_hh, wq)
    if not decoder_step_heightmap_supported(Ks, C, W, L, m, Hd):
        raise ValueError("no height-map decoder-step kernel for Ks %d, C %d, W %d, L %d, m %d, Hd %d (Hd 64 / 128 / 256, m = Hd / 2 or Hd, "
                         "C 1 / 2 / 4, W and L <= 12, Ks <= 16, Ks + m <= Hd + 16)" % (Ks, C, W, L, m, Hd))
    drop, dev = _step_record_on(dropout, P)
    enc_w = (convs[0].weight.reshape(m // 4, C), convs[0].bias, convs[1].weight.reshape(m // 2, m // 4), convs[1].bias,
             convs[2].weight.reshape(m, (m // 2) * nw * nl), convs[2].bias)
    args = [_prep_f32(v, dev) for v in (xs, hm, h) + enc_w + (P, c, w_hh, b_hh, wq)]
    if torch.is_grad_enabled() and any(v is not None and v.requires_grad for v in args):
        return _DecoderStepHeightmap.apply(*args, drop)
    return _step_no_grad(_decoder_hm_launch, args, drop, B, Hd, dev)


class PointerHeadPolicy(object):
    """A pointer network's decoding head as a policy for ``run_episode`` and the steppers (model.py:356-372):
    ``scorer(step=, static=, dynamic=, current_mask=, mask=, decoder_static=, decoder_dynamic=)`` returns the logits
    (B, nR), and ``pointer_pick(logits, current_mask, ...)`` turns them into the step's ptr and log-probability.
    ``u``: PRE-DRAWN uniforms (steps, B) in [0, 1), step-major so a step's row is contiguous (like TapePolicy's tour):
    the episode is then deterministic given ``u`` and can be captured in a hipGraph and replayed on refreshed uniforms.
    ``greedy=True``: the first maximum instead (the reference's test mode).  With neither, ``torch.rand(B,
    generator=generator)`` is drawn per step, eagerly.  ``PointerHeadPolicy.from_source(scorer, source)`` (``source`` a
    ``tools.StepDropout``): the uniform is drawn inside the head's launch from the source's next pick record
    (``pointer_pick_draw``) -- no tensor of uniforms, capturable, new draws on every replay.  Each step's logp is kept: ``tour_logp()`` -> (B, steps), the
    reference's tour_logp (model.py:513); ``reset()`` clears the kept values (step 0 of a new episode does too)."""

    def __init__(self, scorer, u=None, greedy=False, generator=None):
        if greedy and u is not None:
            raise ValueError("greedy=True takes no uniforms")
        self.scorer = scorer
        self.u = u
        self.greedy = bool(greedy)
        self.generator = generator
        self.source = None
        self._logp = []

    @classmethod
    def from_source(cls, scorer, source):
        """the policy that draws inside the head's launch: ``source`` a ``tools.StepDropout`` (anything with ``take_pick()``)"""
        if not hasattr(source, "take_pick"):
            raise TypeError("source must hand out pick records (tools.StepDropout), got %r" % (source,))
        pol = cls(scorer)
        pol.source = source
        return pol

    def reset(self):
        self._logp = []

    def __call__(self, step, current_mask, **kw):
        if step == 0:
            self._logp = []
        logits = self.scorer(step=step, current_mask=current_mask, **kw)
        if self.source is not None:
            ptr, logp = pointer_pick_draw(logits, current_mask, self.source)
        else:
            if self.greedy:
                u = None
            elif self.u is not None:
                u = self.u[step]
            else:
                u = torch.rand(int(logits.shape[0]), generator=self.generator, device=logits.device)
            ptr, logp = pointer_pick(logits, current_mask, u)
        while len(self._logp) <= step:
            self._logp.append(None)
        self._logp[step] = logp
        return ptr

    def tour_logp(self):
        """(B, steps) float32: the kept log-probabilities of the picks, in step order"""
        if not self._logp or any(v is None for v in self._logp):
            raise RuntimeError("PointerHeadPolicy.tour_logp: no complete episode has been kept")
        return torch.stack(self._logp, dim=1)


def _flagged_reward(reward, check, *envs):
    """What an episode reports for containers whose sticky error word is set (a placement above the container's
    height -- the reference's IndexError --, a block the container cannot take, a footprint beyond the big-container
    kernels' support masks, tapenv.h: tap_env_errors): their placements were skipped, so their score is not the
    episode's.  check='nan' (default): NaN reward for exactly those containers, no host sync (two small launches,
    capturable in a hipGraph); 'raise': env.check() -- one host sync, TapOverflowError / TapError like the reference's
    raise; False / None: the raw calc_ratio (the caller checks, e.g. once per epoch with stepper.check())."""
    if not check:
        return reward
    if check == 'raise':
        for e in envs:
            e.check()
        return reward
    if check != 'nan':
        raise ValueError("check must be 'nan', 'raise' or False, not %r" % (check,))
    err = envs[0].errors
    for e in envs[1:]:
        err = err | e.errors
    return torch.where(err != 0, torch.full_like(reward, float('nan')), reward)


def run_episode(static, dynamic, policy, container_width, container_height,
                reward_type='C+P+S-lb-soft', heightmap_type='diff', packing_strategy='LB_GREEDY',
                input_type='bot', allow_rot=True, env=None, record=False, steps=None, fused=True, bits=None,
                container_length=None, stepper=None, check='nan', pack_policy=None, pack_rnn=None):
    """One episode for a batch (model.py:254-515 minus the network).

    ``policy(step=, static=, dynamic=, current_mask=, mask=, decoder_static=, decoder_dynamic=)``
    returns ptr (B,) int64.  With ``fused`` every step is ONE launch (tap_transition*; the two launches behind the
    same entry for the shapes without a single kernel), the first one starting from a fresh container and the last
    one emitting calc_ratio; otherwise a step is two launches (tap_mask_step, tap_env_step_gather).  Returns a dict:
    tour_idx (B, steps), reward = -scores (B,) fp32 (model.py:515), env, and with ``record`` the per-step features /
    masks.  ``bits``: carry ``dynamic`` as its bit shadow between the steps, None = when possible.

    The fused loop runs on a ``pack.EpisodeStepper`` (windows without a bit shadow: on its fp32-copy form): between two calls of the
    policy the host makes ONE C call and issues no torch op (the step's launch also writes ``decoder_static`` and
    the tour column).  ``stepper``: a stepper to re-use across episodes (a trainer builds one per run: nothing is
    allocated per episode; the returned tensors are then views of its buffers, valid until its next ``begin``);
    None builds one for this call.  ``check``: what ``reward`` holds for containers that raised an error bit
    (_flagged_reward: 'nan' -- NaN, no host sync --, 'raise', or False for the raw ratio).

    ``pack_policy(pnet_input, block)``: the learned local pack-net's loop instead (DRL_L.forward, model.py:1016-1250):
    the block goes to a column the pack policy picks -- see _run_episode_pack.

    ``pack_rnn`` (a tools.PackRNN): the global pack-net's loop instead (DRL_RNN.forward, model.py:749-852) -- see
    _run_episode_rnn.
    """
    if pack_rnn is not None:
        if pack_policy is not None:
            raise ValueError("pack_policy and pack_rnn select two different loops")
        return _run_episode_rnn(static, dynamic, policy, pack_rnn, container_width, reward_type, heightmap_type,
                                input_type, allow_rot, record, steps, bits=False if bits is None else bits, check=check)
    if pack_policy is not None:
        return _run_episode_pack(static, dynamic, policy, pack_policy, container_width, container_height, reward_type,
                                 heightmap_type, packing_strategy, input_type, allow_rot, env, record, steps,
                                 bits=False if bits is None else bits, check=check)
    if input_type in ('mul', 'mul-with'):
        return _run_episode_mul(static, dynamic, policy, container_width, container_height, reward_type,
                                heightmap_type, packing_strategy, input_type, allow_rot, record, steps, check)
    block_dim = int(static.shape[1]) - 1
    n = int(dynamic.shape[-1]) // (math.factorial(block_dim) if allow_rot else 1)
    B, D = int(static.shape[0]), block_dim
    nsteps = n if steps is None else steps
    dev = _lib.resolve_device(static.device)
    # (windows without a bit shadow -- rows > 128, nR % 4 != 0, nR > 256 -- run on the stepper too since round 5: its
    #  fp32-copy form; ``bits=True`` still asks for the shadow and fails there)
    if stepper is not None or (fused and bits is not False and not isinstance(bits, torch.Tensor) and
                               (bits is None or bits_supported(int(dynamic.shape[1]), int(dynamic.shape[2])))):
        try:
            return _run_episode_stepper(static, dynamic, policy, container_width, container_height, reward_type,
                                        heightmap_type, packing_strategy, input_type, allow_rot, env, record, nsteps,
                                        container_length, stepper, dev, n, D, check)
        except NonBinaryDynamic:
            if bits is True or stepper is not None:
                raise ValueError("dynamic cannot be carried as a bit shadow (it holds values other than 0 and 1)")
            if env is not None:
                env.reset()
    # model.py:279 builds square 3D containers (L = W); container_length lifts that for callers that want it
    cs = [container_width, container_height] if D == 2 else \
        [container_width, container_length or container_width, container_height]
    if env is None:
        env = BatchedContainer(B, cs, n, reward_type, heightmap_type, packing_strategy=packing_strategy, device=dev)
    if fused:
        masks = EnvTransition(static.to(dev), dynamic.to(dev), env, input_type, allow_rot, bits)
    else:
        masks = MaskStepper(static.to(dev), dynamic.to(dev), input_type, allow_rot, bits)
        env.reset()
    static_part = masks.static[:, 1:, :]
    decoder_static = torch.zeros(B, D, 1, device=dev)
    decoder_dynamic = torch.zeros(env._feature_shape(), device=dev)
    tour, feats, curs, msks = [], [], [], []
    ratio = None
    for step in range(nsteps):
        ptr = policy(step=step, static=masks.static, dynamic=masks.dynamic,
                     current_mask=masks.current_mask, mask=masks.mask,
                     decoder_static=decoder_static, decoder_dynamic=decoder_dynamic)
        ptr = ptr.to(torch.int64)
        decoder_static = torch.gather(static_part, 2, ptr.view(-1, 1, 1).expand(-1, D, 1))  # model.py:404-406
        if fused:                                                 # model.py:376-386 + 451-465, one launch
            _, _, _, decoder_dynamic, r = masks.step(ptr, fresh=(step == 0), want_ratio=(step == nsteps - 1))
            ratio = r if r is not None else ratio
        else:
            masks.step(ptr)                                       # model.py:376-386
            decoder_dynamic = env.add_new_blocks_gather(masks.static, ptr)                  # model.py:451-465
        tour.append(ptr.unsqueeze(1))
        if record:
            feats.append(decoder_dynamic); curs.append(masks.current_mask); msks.append(masks.mask)
    if ratio is None:
        ratio = env.calc_ratios()                                 # model.py:499-510
    out = {'tour_idx': torch.cat(tour, dim=1), 'reward': _flagged_reward(-ratio, check, env), 'env': env,
           'dynamic': masks.dynamic, 'mask': masks.mask}
    if record:
        out.update(features=feats, current_masks=curs, masks=msks)
    return out


def _run_episode_pack(static, dynamic, policy, pack_policy, container_width, container_height, reward_type,
                      heightmap_type, packing_strategy, input_type, allow_rot, env, record, steps, bits=False, check='nan'):
    """DRL_L's decoding loop (model.py:1016-1250) minus its two networks.  Per step: the precedence update
    (tap_mask_step, model.py:1118-1128), ``policy`` -> ptr, ``pack_policy(pnet_input, block)`` -> the column, then one
    place-at launch with the gather fused (tap_env_step_at_gather, Container.add_new_block_at's rules,
    model.py:1205-1212) that also writes the decoder feature and the pack policy's next input.
    ``pnet_input`` (B, 1, W) f32 is the height-map in DRL_L's heightmap_type form (model.py:1180-1196; 'diff' with its
    trailing 0), ``block`` = decoder_static transposed, (B, 1, 2).  pack_policy returns columns (B,) int64, or
    probabilities (B, W), which are argmaxed (model.py:1200-1202) and give ``pack_logp``, the log of the chosen
    column's probability.  A tools.DQN with ``fused`` set is asked through its ``pick`` instead (one launch: the column and
    ``pack_logp``).  Nothing is read back to the host inside the loop, so the episode can be captured in a
    hipGraph.  Returns run_episode's dict plus ``place_x`` (B, steps) int64 [and ``pack_logp`` (B, steps)]."""
    if input_type in ('mul', 'mul-with'):
        raise NotImplementedError("the pack-net loop of the two-container input types is not implemented")
    D = int(static.shape[1]) - 1
    if D != 2:
        raise NotImplementedError("the pack-net placement is 2D only (tools.py:3762 unpacks two block sides)")
    n = int(dynamic.shape[-1]) // (math.factorial(D) if allow_rot else 1)
    B = int(static.shape[0])
    nsteps = n if steps is None else steps
    dev = _lib.resolve_device(static.device)
    if env is None:
        env = BatchedContainer(B, [container_width, container_height], n, reward_type, heightmap_type,
                               packing_strategy=packing_strategy, device=dev, place_at='container')
    elif env.place_at != 'container':
        raise ValueError("env must be a BatchedContainer built with place_at='container'")
    else:
        env.reset()
    masks = MaskStepper(static.to(dev), dynamic.to(dev), input_type, allow_rot, bits)
    static_part = masks.static[:, 1:, :]
    W = env.desc.W
    # two buffers for the pack policy's input, alternating: the one a policy was handed is not overwritten by the step
    # that follows it, but by the one after that -- while grad is enabled the pack policy gets a private copy
    # (pack.grad_copies), so a network that saves its input for backward() keeps this step's height-map
    pnet = [torch.zeros(B, 1, W, dtype=torch.float32, device=dev) for _ in range(2)]
    decoder_static = torch.zeros(B, D, 1, device=dev)
    decoder_dynamic = torch.zeros(env._feature_shape(), device=dev)
    tour, xs, logps, feats, curs, msks, pins = [], [], [], [], [], [], []
    from .tools import DQN
    fused_pick = isinstance(pack_policy, DQN) and pack_policy.fused
    for step in range(nsteps):
        ptr = policy(step=step, static=masks.static, dynamic=masks.dynamic, current_mask=masks.current_mask,
                     mask=masks.mask, decoder_static=decoder_static, decoder_dynamic=decoder_dynamic).to(torch.int64)
        masks.step(ptr)                                                                     # model.py:1118-1128
        decoder_static = torch.gather(static_part, 2, ptr.view(-1, 1, 1).expand(-1, D, 1))  # model.py:1164-1167
        pin, pout = pnet[step % 2], pnet[(step + 1) % 2]
        if torch.is_grad_enabled():
            pin, = grad_copies(pin)
        if fused_pick:                                                                      # tools.DQN.pick: one launch
            out, lp = pack_policy.pick(pin, decoder_static.transpose(2, 1))
            logps.append(lp.unsqueeze(1))
        else:
            out = pack_policy(pin, decoder_static.transpose(2, 1))
        if out.dim() == 2:                                                                  # probabilities, model.py:1200-1202
            best = out.max(1)
            x = best[1]
            logps.append(best[0].log().unsqueeze(1))
        else:
            x = out.reshape(B).to(torch.int64)
        decoder_dynamic = env.add_new_blocks_at_gather(masks.static, ptr, x, pnet_out=pout, pnet_form=heightmap_type)
        tour.append(ptr.unsqueeze(1))
        xs.append(x.unsqueeze(1))
        if record:
            feats.append(decoder_dynamic); curs.append(masks.current_mask); msks.append(masks.mask); pins.append(pin.clone())
    ratio = env.calc_ratios()                                                               # model.py:1226-1234
    out = {'tour_idx': torch.cat(tour, dim=1), 'place_x': torch.cat(xs, dim=1), 'reward': _flagged_reward(-ratio, check, env),
           'env': env, 'dynamic': masks.dynamic, 'mask': masks.mask}
    if logps:
        out['pack_logp'] = torch.cat(logps, dim=1)
    if record:
        out.update(features=feats, current_masks=curs, masks=msks, pnet_inputs=pins)
    return out


# ---- the global pack-net's forward in one launch (tapenv.h: tap_pack_rnn_forward has the contract) ----------------------
def pack_rnn_forward_supported(Hb, Hh, W, kind='G'):
    """whether tap_pack_rnn_forward has a kernel for this net: Hb = Hh = 128, G or LG, 2 <= W <= 64"""
    return int(Hb) == 128 and int(Hh) == 128 and kind in ('G', 'LG') and 2 <= int(W) <= 64


def _pack_rnn_blocks(fold, engine, blocks, blocks_num):
    B, n = int(engine.batch_size), int(blocks_num)
    if blocks.dim() != 3 or int(blocks.shape[0]) != B or int(blocks.shape[1]) != 2:
        raise ValueError("blocks must be (%d, 2, T), got %s" % (B, tuple(blocks.shape)))
    T = int(blocks.shape[2])
    if not 1 <= n <= T or T > int(engine.T):
        raise ValueError("blocks_num %d of %d blocks on a tape of %d" % (n, T, engine.T))
    if engine.heightmap_type != fold.heightmap_type or int(engine.W) != fold.W:
        raise ValueError("the engine is %d columns / %r, the net was folded for %d / %r"
                         % (engine.W, engine.heightmap_type, fold.W, fold.heightmap_type))
    return B, n, T


def pack_rnn_forward(fold, engine, blocks, blocks_num, want_input=True):
    """PackRNN.forward's eval form in ONE launch (tap_pack_rnn_forward): ``fold`` a ``tools.PackFold`` of float32 tensors on
    the GPU (``tools.PackRNN.fold``), ``engine`` an ``env.PackEngines``, ``blocks`` (B, 2, T) float32 on its device.
    -> hit_porb_log (B, blocks_num) float32 and the net's next input (B, W', 1) (None without ``want_input``); the engine's
    blob, tape, error words and ``reward`` hold what ``blocks_num`` ``engine.step`` calls at the picked columns leave.
    No allocation beyond the two outputs, no host read: capturable."""
    from .env import PackEngines
    if not isinstance(engine, PackEngines):
        raise TypeError("the fused forward steps an env.PackEngines, not %s" % type(engine).__name__)
    B, n, T = _pack_rnn_blocks(fold, engine, blocks, blocks_num)
    if not pack_rnn_forward_supported(fold.Hb, fold.Hh, fold.W, fold.kind):
        raise _lib.TapError(_lib.TAP_E_UNSUPPORTED, "no pack-net kernel for Hb %d, Hh %d, W %d, kind %r" % (fold.Hb, fold.Hh, fold.W, fold.kind))
    blocks = engine._blocks(blocks.detach())
    w = fold.weights(engine.device)
    logp = torch.empty(B, n, dtype=torch.float32, device=engine.device)
    feat = engine.env._new_feature() if want_input else None
    engine.env._call(_lib.lib().tap_pack_rnn_forward, _lib.ptr(engine.env._state), _lib.ptr(blocks), T, n, engine.max_blocks_num,
                     _lib.C.byref(w), _lib.ptr(logp), _lib.ptr(engine.reward), _lib.ptr(feat))
    engine.last_input = feat
    return logp, feat


def pack_rnn_forward_torch(fold, engine, blocks, blocks_num, want_input=True):
    """``pack_rnn_forward``'s contract in torch ops, in ``blocks``' dtype (the fold's): the folded algebra, the chains as
    matmuls, ``engine`` anything with PackEngines' surface.  In float64 it is the model the launch is tested against."""
    B, n, T = _pack_rnn_blocks(fold, engine, blocks, blocks_num)
    f, dt, dev = fold, blocks.dtype, blocks.device
    blocks = blocks.detach()

    def cell(gi, gh, h, H):
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        nn_ = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        return (1 - z) * nn_ + z * h
    h = torch.zeros(B, f.Hb, dtype=dt, device=dev)
    for t in range(T):                                                       # all T columns (LG_RL.py:603-620)
        h = cell(blocks[:, :, t] @ f.Pe.t() + f.ce, h @ f.enc_w_hh.t() + f.enc_b_hh, h, f.Hb)
    u = h @ f.Pd_e.t() + f.cd
    hd = torch.zeros(B, f.D, dtype=dt, device=dev)
    x = torch.zeros(B, f.Wp, dtype=dt, device=dev)
    logps, feat = [], None
    for i in range(n):
        gi = u
        if f.kind == 'LG':
            gi = gi + blocks[:, :, i] @ f.Pd_b.t()
        gi = gi + x @ f.Pd_h.t()
        hd = cell(gi, hd @ f.dec_w_hh.t() + f.dec_b_hh, hd, f.D)
        logit = torch.relu(hd @ f.fc0_w.t() + f.fc0_b) @ f.fc2_w.t() + f.fc2_b
        m, col = logit.max(1)                                                # the first maximum (LG_RL.py:659)
        s = torch.exp((logit - m.unsqueeze(1)).double()).sum(1)
        logps.append((-torch.log(s)).to(dt).unsqueeze(1))
        last = i == n - 1
        feat = engine.step(i, blocks, col, want_reward=last, want_input=want_input or not last)
        if feat is not None:
            x = feat.to(dt)[:, :, 0]
    return torch.cat(logps, dim=1), feat


# ---- the local pack-net's pick in one launch (tapenv.h: tap_dqn_pick has the contract) ----------------------------------
def dqn_pick_supported(W, is_diff_height):
    """whether tap_dqn_pick has a kernel for this net: W >= 2 and at most 14 positions (W <= 12, 13 in the diff form)"""
    return _lib.dqn_pick_geometry(W, is_diff_height) is not None


def _dqn_rows(fold, pnet, block):
    """the two inputs as (B, >= Wm) and (B, 2) views: (B, 1, W) / (B, 1, 2) as DQN.forward takes them, or without the
    middle axis"""
    if pnet.dim() == 3 and pnet.shape[1] == 1:
        pnet = pnet[:, 0]
    if block.dim() == 3 and block.shape[1] == 1:
        block = block[:, 0]
    B = int(pnet.shape[0])
    if pnet.dim() != 2 or block.dim() != 2 or int(block.shape[0]) != B or int(block.shape[1]) != 2 or \
            int(pnet.shape[1]) != fold.W:
        raise ValueError("the pack-net of %d columns takes a map (B, 1, %d) and a block (B, 1, 2), got %s and %s"
                         % (fold.W, fold.W, tuple(pnet.shape), tuple(block.shape)))
    return B, pnet, block


def _dqn_view(t):
    """t (B, k) as the launch reads it -- unit stride along a row, any env stride: the tensor itself where its strides allow"""
    t = t.detach()
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):
        t = t.contiguous()
    elif t.shape[0] <= 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]))


def dqn_pick(fold, pnet, block, want_probs=False):
    """DQN.forward's eval form and the pick in ONE launch (tap_dqn_pick): ``fold`` a ``tools.DqnFold`` of float32 tensors on
    the GPU (``tools.DQN.fold``), ``pnet`` (B, 1, W) the map as DQN.forward takes it (the diff form's trailing entry is
    never read), ``block`` (B, 1, 2), both float32 on the fold's device; views with a unit last stride are read in place
    (``blocks_f[:, t:t + 1, :]``).  -> x (B,) int64 the first column of the largest probability, logp (B,) float32 its log
    [, probs (B, W) float32].  No allocation beyond the outputs, no host read: capturable."""
    B, pnet, block = _dqn_rows(fold, pnet, block)
    if not dqn_pick_supported(fold.W, fold.is_diff_height):
        raise _lib.TapError(_lib.TAP_E_UNSUPPORTED, "no pack-net pick kernel for W %d, diff %r" % (fold.W, fold.is_diff_height))
    if pnet.dtype != torch.float32 or block.dtype != torch.float32:
        raise TypeError("the fused pick takes float32 inputs, got %s and %s" % (pnet.dtype, block.dtype))
    dev = _lib.resolve_device(pnet.device)
    if block.device != pnet.device:
        raise ValueError("the map is on %s, the block on %s" % (pnet.device, block.device))
    w = fold.weights(dev)
    pnet, ps = _dqn_view(pnet)
    block, bs = _dqn_view(block)
    x = torch.empty(B, dtype=torch.int64, device=dev)
    logp = torch.empty(B, dtype=torch.float32, device=dev)
    probs = torch.empty(B, fold.W, dtype=torch.float32, device=dev) if want_probs else None
    c = _lib.ctx(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().tap_dqn_pick(c, _lib.C.byref(w), _lib.ptr(pnet), ps, _lib.ptr(block), bs, B, _lib.ptr(x), _lib.ptr(logp),
                                           _lib.ptr(probs), _lib.stream_of(dev)), c)
    return (x, logp, probs) if want_probs else (x, logp)


def dqn_pick_torch(fold, pnet, block, want_probs=False):
    """``dqn_pick``'s contract in torch ops, in the fold's dtype on its device: the same fold, the same term order (lin1 over
    k = p * 256 + c), the chains as matmuls.  In float64 it is the model the launch is tested against."""
    B, pnet, block = _dqn_rows(fold, pnet, block)
    f, dt = fold, fold.W2.dtype
    xm, xb = pnet[:, :f.Wm].to(dt).unsqueeze(2), block.to(dt).unsqueeze(2)                    # (B, Wm, 1), (B, 2, 1)
    h = torch.relu(torch.cat((f.a_m * xm + f.b_m, f.a_b * xb + f.b_b), 1))                      # (B, P, 128)
    h = torch.relu(h @ f.W2.t() + f.b2)
    h = torch.relu(h @ f.W3.t() + f.b3)
    y = torch.relu(h.reshape(B, f.P * 256) @ f.L1.t() + f.l1b)
    logit = y @ f.head_w.t() + f.head_b
    m, x = logit.max(1)                                                      # the first maximum
    e = torch.exp((logit - m.unsqueeze(1)).double())
    s = e.sum(1)
    logp = (-torch.log(s)).to(dt)
    return (x, logp, (e / s.unsqueeze(1)).to(dt)) if want_probs else (x, logp)


def _run_episode_rnn(static, dynamic, policy, net, container_width, reward_type, heightmap_type, input_type, allow_rot,
                     record, steps, bits=False, check='nan'):
    """DRL_RNN's decoding loop (model.py:749-852) minus its pointer network.  Per outer step t: ``policy`` -> ptr, the
    precedence update (tap_mask_step), the gather of decoder_static (model.py:801-803), then ``net`` re-packs the whole
    prefix of t + 1 chosen blocks from an empty container (model.py:809-811: t + 1 engine launches,
    (n + 1) n / 2 in an episode), and decoder_dynamic is the engines' height-map in ``heightmap_type`` form after that
    forward (model.py:814-826; (B, W', 1)).  Nothing is read back to the host inside the loop, so the episode can be
    captured in a hipGraph.  Returns tour_idx (B, steps), reward = DRL_RNN's ``scores`` (the last forward's -rw, (B,)
    float32), pack_logp = the last forward's hit_porb_log (B, steps), place_x (B, steps) int64 = the last forward's
    columns, the engine (net's) [and with ``record`` the per-step decoder_dynamic as ``features``].  An episode
    captured in a hipGraph writes that engine's state blob on every replay: the net keeps it alive
    (net.captured_engines) even after a call with another batch size replaced net's current engine."""
    if input_type in ('mul', 'mul-with'):
        raise NotImplementedError("the pack-net loop of the two-container input types is not implemented")
    D = int(static.shape[1]) - 1
    if D != 2:
        raise NotImplementedError("the global pack-net is 2D only (PackEngine's height-map is a row)")
    if int(net.container_width) != int(container_width):
        raise ValueError("the pack-net places into %d columns, the episode has %d" % (net.container_width, container_width))
    n = int(dynamic.shape[-1]) // (math.factorial(D) if allow_rot else 1)
    nsteps = n if steps is None else steps
    dev = _lib.resolve_device(static.device)
    masks = MaskStepper(static.to(dev), dynamic.to(dev), input_type, allow_rot, bits)
    return rnn_loop(policy, masks, net, heightmap_type, nsteps, record, check)


def rnn_loop(policy, masks, net, heightmap_type, nsteps, record=False, check='nan'):
    """The body of _run_episode_rnn on a given precedence stepper ``masks`` (a MaskStepper, or any object with its
    static / dynamic / current_mask / mask attributes and step(ptr)); the engine is ``net``'s own."""
    B, D = int(masks.static.shape[0]), int(masks.static.shape[1]) - 1
    dev = masks.static.device
    engine = net.reserve(B, nsteps, dev)
    static_part = masks.static[:, 1:, :]
    W = int(net.container_width)
    decoder_static = torch.zeros(B, D, 1, device=dev)
    decoder_dynamic = torch.zeros(B, W - 1 if heightmap_type == 'diff' else W, 1, device=dev)
    tour, all_blocks, feats = [], [], []
    pack_logp = scores = positions = None
    for step in range(nsteps):
        ptr = policy(step=step, static=masks.static, dynamic=masks.dynamic, current_mask=masks.current_mask,
                     mask=masks.mask, decoder_static=decoder_static, decoder_dynamic=decoder_dynamic).to(torch.int64)
        masks.step(ptr)                                                                     # model.py:784-793
        decoder_static = torch.gather(static_part, 2, ptr.view(-1, 1, 1).expand(-1, D, 1))  # model.py:801-803
        all_blocks.append(decoder_static)
        pack_blocks = torch.cat(all_blocks, dim=-1)                                         # model.py:810
        positions, pack_logp, scores = net(pack_blocks, step + 1)                           # model.py:811
        decoder_dynamic = engine.get_heightaps(heightmap_type)                              # model.py:816-826
        tour.append(ptr.unsqueeze(1))
        if record:
            feats.append(decoder_dynamic)
    out = {'tour_idx': torch.cat(tour, dim=1), 'reward': _flagged_reward(scores.detach(), check, engine),
           'pack_logp': pack_logp, 'place_x': positions[:, :nsteps, 0].to(torch.int64), 'engine': engine,
           'dynamic': masks.dynamic, 'mask': masks.mask}
    if record:
        out['features'] = feats
    return out


def _as_instances(t, dev):
    if t.dtype is not torch.float32 or not t.is_contiguous() or t.device != dev:
        t = t.to(device=dev, dtype=torch.float32).contiguous()
    return t


def _run_episode_stepper(static, dynamic, policy, container_width, container_height, reward_type, heightmap_type,
                         packing_strategy, input_type, allow_rot, env, record, nsteps, container_length, stepper, dev, n, D,
                         check='nan'):
    """run_episode's loop on a pack.EpisodeStepper: per decoding step the policy's call and one C call."""
    static, dynamic = _as_instances(static, dev), _as_instances(dynamic, dev)
    if stepper is None:
        if env is None:
            cs = [container_width, container_height] if D == 2 else \
                [container_width, container_length or container_width, container_height]   # model.py:279: L = W
            env = BatchedContainer(int(static.shape[0]), cs, n, reward_type, heightmap_type,
                                   packing_strategy=packing_strategy, device=dev)
        stepper = EpisodeStepper(static, dynamic, env, input_type, allow_rot, steps=nsteps)
    elif stepper.steps != nsteps:
        raise ValueError("the stepper was built for %d steps per episode, not %d" % (stepper.steps, nsteps))
    sp = stepper
    sp.begin(static, dynamic)
    feats, curs, msks = [], [], []
    for step in range(nsteps):
        ptr = policy(step=step, static=static, dynamic=sp.dynamic, current_mask=sp.current_mask, mask=sp.mask,
                     decoder_static=sp.decoder_static, decoder_dynamic=sp.decoder_dynamic)
        sp.step(ptr)                                              # model.py:376-465, one launch
        if record:
            feats.append(sp.decoder_dynamic.clone()); curs.append(sp.current_mask.clone()); msks.append(sp.mask.clone())
    out = {'tour_idx': sp.tour, 'reward': _flagged_reward(-sp.ratio, check, sp.env), 'env': sp.env, 'dynamic': sp.dynamic,
           'mask': sp.mask, 'stepper': sp}
    if record:
        out.update(features=feats, current_masks=curs, masks=msks)
    return out


def _run_episode_mul(static, dynamic, policy, container_width, container_height, reward_type,
                     heightmap_type, packing_strategy, input_type, allow_rot, record, steps, check='nan'):
    """The two-container variant (input types 'mul' / 'mul-with', model.py:290-292, 396-447,
    503-507): the last row of ``static`` holds each block's target container id; per step the chosen
    block is placed in container a (id 0) or b (id 1) and the other one only reports its height-map
    (the C ABI's ``active`` mask); decoder features are concatenated on dim 1 and the score is the
    mean of the two ``calc_ratio`` values."""
    D = int(static.shape[1]) - 2
    n = int(dynamic.shape[-1]) // (math.factorial(D) if allow_rot else 1)
    B = int(static.shape[0])
    cs = [container_width, container_height] if D == 2 else [container_width, container_width, container_height]
    dev = _lib.resolve_device(static.device)
    env_a = BatchedContainer(B, cs, n, reward_type, heightmap_type, packing_strategy=packing_strategy, device=dev)
    env_b = BatchedContainer(B, cs, n, reward_type, heightmap_type, packing_strategy=packing_strategy, device=dev)
    masks = MaskStepper(static.to(dev), dynamic.to(dev), input_type, allow_rot)
    static_part = masks.static[:, 1:-1, :] if input_type == 'mul' else masks.static[:, 1:, :]   # model.py:389-394
    ssize = static_part.shape[1]
    decoder_static = torch.zeros(B, ssize, 1, device=dev)
    decoder_dynamic = torch.cat((torch.zeros(env_a._feature_shape(), device=dev),
                                 torch.zeros(env_b._feature_shape(), device=dev)), 1)
    tour, feats, curs, msks = [], [], [], []
    for step in range(n if steps is None else steps):
        ptr = policy(step=step, static=masks.static, dynamic=masks.dynamic,
                     current_mask=masks.current_mask, mask=masks.mask,
                     decoder_static=decoder_static, decoder_dynamic=decoder_dynamic).to(torch.int64)
        masks.step(ptr)
        target = torch.gather(masks.static[:, -1, :], 1, ptr.view(-1, 1)).squeeze(1)           # model.py:396-401
        decoder_static = torch.gather(static_part, 2, ptr.view(-1, 1, 1).expand(-1, ssize, 1))
        fa = env_a.add_new_blocks_gather(masks.static, ptr, active=(target == 0))               # model.py:419-427
        fb = env_b.add_new_blocks_gather(masks.static, ptr, active=(target == 1))
        decoder_dynamic = torch.cat((fa, fb), 1)                                               # model.py:429-447
        tour.append(ptr.unsqueeze(1))
        if record:
            feats.append(decoder_dynamic); curs.append(masks.current_mask); msks.append(masks.mask)
    ratio = (env_a.calc_ratios() + env_b.calc_ratios()) / 2.0                                  # model.py:503-507
    out = {'tour_idx': torch.cat(tour, dim=1), 'reward': _flagged_reward(-ratio, check, env_a, env_b), 'env': env_a, 'env_b': env_b,
           'dynamic': masks.dynamic, 'mask': masks.mask}
    if record:
        out.update(features=feats, current_masks=curs, masks=msks)
    return out
