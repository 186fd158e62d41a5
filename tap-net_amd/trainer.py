"""The reference's trainer (trainer.py:96-313) on this package: ``validate``, ``train`` and, between them and the modules,
one training iteration as an object (``TrainStep``).  The tail of the iteration -- the advantage, both losses, both
``clip_grad_norm_`` calls and both ``Adam.step()`` calls, trainer.py:216-236 -- is three launches of csrc/train.hip
(``reinforce_seeds``, ``ClipAdam.step``) that read nothing on the host, so the whole iteration can be replayed from one
graph.  DESIGN 7o has the contracts; INTEGRATION 2o the binding.

Off the GPU, and for a dtype other than float32, every piece here is the same arithmetic in torch ops in the tensors' own
dtype: in float64 that is the model the device path is tested against."""
import datetime
import os
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import _lib, pack

__all__ = ["ClipAdam", "TrainStep", "reinforce_losses", "reinforce_seeds", "train", "validate"]

DEFAULT_CHUNK = 4096          # elements per table entry: a workgroup's 256 threads take four 16-byte quads each
# What TrainStep and train() do unless told otherwise; set by profiles/trainer.json (scripts/time_trainer.py), DESIGN 7o.
DEFAULT_TAIL = 'hip'
DEFAULT_GRAPH = True

_CHUNK_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("count", "<i4"), ("group", "<i4")])
assert _CHUNK_DTYPE.itemsize == 40                                         # tapenv.h: tap_adam_chunk


def _on_device(*tensors):
    return all(t.is_cuda and t.dtype is torch.float32 for t in tensors)


# ---- the losses ---------------------------------------------------------------------------------------------------------
_scratch = {}


def _losses_scratch(dev, B):
    need = int(_lib.lib().tap_reinforce_losses_scratch(B))
    key = (dev.index, need)
    if key not in _scratch:
        _scratch[key] = torch.zeros(need // 8, dtype=torch.int64, device=dev)   # zeroed once: the launches keep the ticket at 0
    return _scratch[key], need


def _seeds_torch(reward, critic_est, tour_logp):
    B = int(reward.shape[0])
    ok = torch.isfinite(reward)
    zero = torch.zeros_like(reward)
    adv = torch.where(ok, reward - critic_est, zero)
    seed_logp = (adv / B).unsqueeze(1).expand(B, int(tour_logp.shape[1])).contiguous()
    seed_est = torch.where(ok, (-2 * adv) / B, zero)
    advd, row = adv.double(), tour_logp.double().sum(1)
    stats = torch.stack([(advd * row).sum() / B, (advd * advd).sum() / B, torch.where(ok, reward, zero).double().sum() / B,
                         torch.where(ok, critic_est, zero).double().sum() / B, (~ok).sum().double()]).to(reward.dtype)
    return adv, seed_logp, seed_est, stats


def reinforce_seeds(reward, critic_est, tour_logp):
    """trainer.py:216-225 -> (adv (B,), seed_logp (B, n), seed_est (B,), stats (5,)), nothing of it under autograd.
    adv = reward - critic_est; seed_logp = adv / B in every column, the gradient of ``mean(adv.detach() * tour_logp.sum(1))``;
    seed_est = -2 adv / B, the gradient of ``mean(adv ** 2)`` with respect to ``critic_est``; stats = actor_loss,
    critic_loss, mean reward, mean critic_est, flagged envs.  An env whose reward is not finite -- a flagged container under
    ``check='nan'`` -- has adv = 0 and zero seeds, is left out of the four sums and is counted; the divisor stays B.
    float32 tensors on the GPU: ONE launch (tapenv.h: tap_reinforce_losses), the same bytes on every call; elsewhere the
    same in torch ops."""
    if tour_logp.dim() != 2 or reward.dim() != 1 or reward.shape != critic_est.shape or tour_logp.shape[0] != reward.shape[0]:
        raise ValueError("reward (B,), critic_est (B,) and tour_logp (B, n) expected, got %s, %s, %s" % (
            tuple(reward.shape), tuple(critic_est.shape), tuple(tour_logp.shape)))
    reward, critic_est, tour_logp = reward.detach(), critic_est.detach(), tour_logp.detach()
    if not _on_device(reward, critic_est, tour_logp):
        with torch.no_grad():
            return _seeds_torch(reward, critic_est, tour_logp)
    dev = reward.device
    B, n = (int(v) for v in tour_logp.shape)
    reward, critic_est, tour_logp = reward.contiguous(), critic_est.contiguous(), tour_logp.contiguous()
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)    # noqa: E731
    adv, seed_logp, seed_est, stats = f(B), f(B, n), f(B), f(5)
    if B == 0:
        return adv, seed_logp, seed_est, stats.zero_()
    scratch, need = _losses_scratch(dev, B)
    c = _lib.ctx(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().tap_reinforce_losses(c, _lib.ptr(reward), _lib.ptr(critic_est), _lib.ptr(tour_logp), B, n, _lib.ptr(adv),
                                                   _lib.ptr(seed_logp), _lib.ptr(seed_est), _lib.ptr(stats), _lib.ptr(scratch), need,
                                                   _lib.stream_of(dev)), c)
    return adv, seed_logp, seed_est, stats


class _ReinforceLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, reward, critic_est, tour_logp):
        _, seed_logp, seed_est, stats = reinforce_seeds(reward, critic_est, tour_logp)
        ctx.save_for_backward(seed_logp, seed_est)
        return stats[0].clone(), stats[1].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_actor, g_critic):
        seed_logp, seed_est = ctx.saved_tensors
        d_est = g_critic * seed_est
        return (-d_est if ctx.needs_input_grad[0] else None, d_est if ctx.needs_input_grad[1] else None,
                g_actor * seed_logp if ctx.needs_input_grad[2] else None)


def reinforce_losses(reward, critic_est, tour_logp):
    """-> (actor_loss, critic_loss) of trainer.py:222 / 225 as scalars under autograd, over ``reinforce_seeds``' launch: the
    backward multiplies the kept seeds by the incoming scalars (``actor_loss`` reaches ``tour_logp`` alone, as through the
    reference's ``advantage.detach()``)."""
    return _ReinforceLosses.apply(reward, critic_est, tour_logp)


# ---- clip_grad_norm_ + Adam ------------------------------------------------------------------------------------------------
class ClipAdam(object):
    """``clip_grad_norm_`` and ``torch.optim.Adam.step()`` for several modules' parameters in two launches (tapenv.h:
    tap_clip_adam_norm / tap_clip_adam_apply).  ``groups``: a list of ``(params, lr, max_norm)``, one per optimizer of the
    loop this replaces -- its own norm, its own clipping, its own step counter.  ``betas``, ``eps``: Adam's; no weight decay,
    no amsgrad.  ``chunk``: elements per entry of the device table (a multiple of 4); a test forces many chunks with it.

    The object owns one flat gradient buffer, one ``exp_avg`` and one ``exp_avg_sq`` buffer per group, slices 16-byte
    aligned, and points every ``p.grad`` at its slice: autograd accumulates in place and no address ever changes, which is
    what lets a captured graph hold them.  Parameters stay the modules' own tensors (contiguous; a view at any element
    offset is fine).  ``step()`` zeroes the gradients unless ``zero_grads=False``.  A group whose norm is not finite is
    skipped -- parameters, moments and counter untouched, gradients zeroed, ``skipped`` one higher -- where the reference
    would carry the NaN into every weight.  lr and max_norm live on the device (``set_lr``): no re-capture for a new value.

    Off the GPU, or for a dtype other than float32, ``step()`` is the same arithmetic in torch ops in the parameters' dtype."""

    def __init__(self, groups, betas=(0.9, 0.999), eps=1e-8, chunk=None, zero_grads=True):
        chunk = DEFAULT_CHUNK if chunk is None else int(chunk)
        if chunk < 4 or chunk % 4:
            raise ValueError("chunk must be a positive multiple of 4, got %d" % chunk)
        self.chunk, self.zero_grads = chunk, bool(zero_grads)
        self.groups = []                    # per group: list of (param, offset, numel)
        self._g, self._m, self._v = [], [], []
        hyper, first = [], None
        for params, lr, max_norm in groups:
            params = [p for p in params if p.numel() > 0]
            if not params:
                raise ValueError("a group without parameters")
            first = params[0] if first is None else first
            slices, off = [], 0
            for p in params:
                if p.device != first.device or p.dtype != first.dtype or not p.is_contiguous():
                    raise ValueError("every parameter must be contiguous, on %s and %s" % (first.device, first.dtype))
                slices.append((p, off, p.numel()))
                off += (p.numel() + 3) // 4 * 4
            flat = lambda: torch.zeros(off, dtype=first.dtype, device=first.device)      # noqa: E731
            g, m, v = flat(), flat(), flat()
            for p, o, k in slices:
                p.grad = g[o:o + k].view_as(p)
            self.groups.append(slices)
            self._g.append(g), self._m.append(m), self._v.append(v)
            hyper.append([float(lr), float(betas[0]), float(betas[1]), float(eps), float(max_norm)])
        self.device, self.dtype = first.device, first.dtype
        self.on_device = self.device.type == 'cuda' and self.dtype is torch.float32
        G = len(self.groups)
        self.hyper = torch.tensor(hyper, dtype=torch.float64).to(self.device)
        self.steps = torch.zeros(G, 2, dtype=torch.int64, device=self.device)             # the counter, the norm launch's snapshot
        self.norms = torch.zeros(G, dtype=torch.float32, device=self.device)
        self._skipped = torch.zeros(G, dtype=torch.int32, device=self.device)
        if self.on_device:
            self._build_table()

    def _build_table(self):
        rows, ranges = [], []
        for gi, slices in enumerate(self.groups):
            start = len(rows)
            g, m, v = (t.data_ptr() for t in (self._g[gi], self._m[gi], self._v[gi]))
            for p, o, k in slices:
                for c0 in range(0, k, self.chunk):
                    rows.append((p.data_ptr() + 4 * c0, g + 4 * (o + c0), m + 4 * (o + c0), v + 4 * (o + c0), min(self.chunk, k - c0), gi))
            ranges.append((start, len(rows) - start))
        table = np.array(rows, dtype=_CHUNK_DTYPE)
        self.nchunks = len(rows)
        self._table = torch.from_numpy(table.view(np.uint8).copy()).to(self.device)
        self._ranges = torch.tensor(ranges, dtype=torch.int32).to(self.device)
        self._partials = torch.zeros(self.nchunks, dtype=torch.float64, device=self.device)

    def views(self, p):
        """-> (grad, exp_avg, exp_avg_sq) of parameter ``p``: views of the flat buffers, shaped like ``p``"""
        for gi, slices in enumerate(self.groups):
            for q, o, k in slices:
                if q is p:
                    return tuple(t[o:o + k].view_as(p) for t in (self._g[gi], self._m[gi], self._v[gi]))
        raise KeyError("not a parameter of this optimizer")

    def set_lr(self, group, lr):
        self.hyper[group, 0] = float(lr)

    @property
    def grad_norm(self):
        """(groups,) float32 on the parameters' device: each group's gradient norm before clipping, at the latest ``step()``"""
        return self.norms

    @property
    def skipped(self):
        """how many group steps were skipped for a norm that was not finite (reads the device)"""
        return int(self._skipped.sum().item())

    def zero_grad(self):
        for g in self._g:
            g.zero_()

    def step(self):
        if not self.on_device:
            return self._step_torch()
        c, L = _lib.ctx(self.device), _lib.lib()
        with torch.cuda.device(self.device):
            st = _lib.stream_of(self.device)
            G = len(self.groups)
            _lib.check(L.tap_clip_adam_norm(c, _lib.ptr(self._table), self.nchunks, G, _lib.ptr(self._ranges), _lib.ptr(self.steps),
                                            _lib.ptr(self._partials), st), c)
            _lib.check(L.tap_clip_adam_apply(c, _lib.ptr(self._table), self.nchunks, G, _lib.ptr(self._ranges), _lib.ptr(self.hyper),
                                             _lib.ptr(self.steps), _lib.ptr(self._partials), _lib.ptr(self.norms), _lib.ptr(self._skipped),
                                             1 if self.zero_grads else 0, st), c)

    @torch.no_grad()
    def _step_torch(self):
        hyper = self.hyper.tolist()
        for gi, slices in enumerate(self.groups):
            lr, b1, b2, eps, max_norm = hyper[gi]
            g, m, v = self._g[gi], self._m[gi], self._v[gi]
            norm = torch.sqrt((g * g).sum())                                   # (the padding between slices is zero)
            self.norms[gi] = norm
            if not bool(torch.isfinite(norm)):
                self._skipped[gi] += 1
            else:
                t = int(self.steps[gi, 0]) + 1
                gc = g * torch.clamp(max_norm / (norm + 1e-6), max=1.0)
                m.mul_(b1).add_(gc, alpha=1 - b1)
                v.mul_(b2).addcmul_(gc, gc, value=1 - b2)
                update = (lr / (1 - b1 ** t)) * (m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps))
                for p, o, k in slices:
                    p.sub_(update[o:o + k].view_as(p))
                self.steps[gi, 0] = t
            if self.zero_grads:
                g.zero_()

    def state_dict(self):
        """the format is this class's own: the flat moments per group, the step counters, the skipped words, the hyper rows"""
        cpu = lambda t: t.detach().cpu().clone()                              # noqa: E731
        return {"exp_avg": [cpu(t) for t in self._m], "exp_avg_sq": [cpu(t) for t in self._v], "steps": cpu(self.steps[:, 0]),
                "skipped": cpu(self._skipped), "hyper": cpu(self.hyper)}

    def load_state_dict(self, sd):
        if len(sd["exp_avg"]) != len(self.groups) or any(a.shape != b.shape for a, b in zip(sd["exp_avg"], self._m)):
            raise ValueError("the state dict is another optimizer's: group sizes differ")
        with torch.no_grad():
            for dst, src in zip(self._m + self._v, list(sd["exp_avg"]) + list(sd["exp_avg_sq"])):
                dst.copy_(src)
            self.steps[:, 0].copy_(sd["steps"])
            self._skipped.copy_(sd["skipped"])
            self.hyper.copy_(sd["hyper"])


# ---- one iteration ---------------------------------------------------------------------------------------------------------
class TrainStep(object):
    """One iteration of the reference's loop (trainer.py:185-236) on an actor (``tools.DRL``) and a critic
    (``tools.StateCritic``).  ``input_type`` and ``packing_strategy`` are read off the actor.  ``step(static, dynamic,
    decoder_static, decoder_dynamic, tour=None, stepper=None)``, in order: ``static_input`` by the reference's slices
    (lines 206-211); the critic on ``pack.dynamic_bits(dynamic)[0]``, the INITIAL shadow (off the GPU: on ``dynamic`` itself);
    ``actor(...)``; ``reinforce_seeds``; ONE ``torch.autograd.backward([tour_logp, critic_est], [seed_logp, seed_est])``;
    ``ClipAdam.step()`` with one group per module.  The modules share no parameter and the actor's seed holds the detached
    advantage, so one backward and one optimizer call give the reference's two backwards and two steps, in its order.
    -> the stats row (``reinforce_seeds``) as a device tensor; nothing is read on the host.

    ``tail='torch'`` keeps the same iteration with stock torch behind the backward: the loss lines in torch ops,
    ``clip_grad_norm_`` and ``torch.optim.Adam`` per module.  ``capture(batch)`` records one iteration on static input buffers
    into one graph (it needs ``pack.set_binary_check('trust')`` and the device tail); ``replay(batch)`` copies a batch in
    and replays it.  The packing strategies 'pre_train' and 'none_train' add the pack-net's log-probabilities to the actor
    loss and need actor modules this package does not have: NotImplementedError."""

    def __init__(self, actor, critic, actor_lr, critic_lr, max_grad_norm, obj_dim, decoder_input_type, tail=None, chunk=None):
        self.input_type, self.packing_strategy = actor.input_type, actor.packing_strategy
        if self.packing_strategy in ('pre_train', 'none_train'):
            raise NotImplementedError("packing_strategy %r: the pack_logp term of the actor loss needs the pack-net actor" % (self.packing_strategy,))
        tail = DEFAULT_TAIL if tail is None else tail
        if tail not in ('hip', 'torch'):
            raise ValueError("tail must be 'hip' or 'torch', not %r" % (tail,))
        self.actor, self.critic, self.tail = actor, critic, tail
        self.obj_dim, self.decoder_input_type, self.max_grad_norm = int(obj_dim), decoder_input_type, float(max_grad_norm)
        if tail == 'hip':
            self.optim = ClipAdam([(list(actor.parameters()), actor_lr, max_grad_norm), (list(critic.parameters()), critic_lr, max_grad_norm)],
                                  chunk=chunk)
        else:
            self.optim = None
            self.actor_optim = torch.optim.Adam(actor.parameters(), lr=actor_lr)
            self.critic_optim = torch.optim.Adam(critic.parameters(), lr=critic_lr)
        self._graph = None

    def forward(self, static, dynamic, decoder_static, decoder_dynamic, tour=None, stepper=None):
        """the iteration up to the backward's inputs -> (tour_logp, critic_est (B,), reward)"""
        if self.input_type == 'mul-with':
            static_input = static[:, 1:, :]
        elif self.input_type == 'rot-old':
            static_input = static
        else:
            static_input = static[:, 1:1 + self.obj_dim, :]
        decoder_input = decoder_static if self.decoder_input_type == 'shape_only' else [decoder_static, decoder_dynamic]
        shadow = pack.dynamic_bits(dynamic)[0] if dynamic.is_cuda else dynamic
        # the critic's drop_hh acts on last_hh alone, which nothing reads (tools.StateCritic): switched off for the call, so
        # torch's generator is never touched -- a graph-registered generator aborts the queue on this stack
        drop = getattr(self.critic, 'drop_hh', None)
        was = drop.training if drop is not None else False
        if was:
            drop.training = False
        try:
            critic_est = self.critic(static_input, shadow).view(-1)
        finally:
            if was:
                drop.training = True
        _, tour_logp, _, reward = self.actor(static, dynamic, decoder_input, tour=tour, stepper=stepper)
        return tour_logp, critic_est, reward

    def step(self, static, dynamic, decoder_static, decoder_dynamic, tour=None, stepper=None):
        tour_logp, critic_est, reward = self.forward(static, dynamic, decoder_static, decoder_dynamic, tour, stepper)
        if self.tail == 'torch':
            return self._torch_tail(tour_logp, critic_est, reward)
        _, seed_logp, seed_est, stats = reinforce_seeds(reward, critic_est, tour_logp)
        torch.autograd.backward([tour_logp, critic_est], [seed_logp, seed_est])
        self.optim.step()
        return stats

    def _torch_tail(self, tour_logp, critic_est, reward):
        with torch.no_grad():
            _, seed_logp, seed_est, stats = _seeds_torch(reward.detach(), critic_est.detach(), tour_logp.detach())
        self.actor_optim.zero_grad()
        self.critic_optim.zero_grad()
        torch.autograd.backward([tour_logp, critic_est], [seed_logp, seed_est])
        torch.nn.utils.clip_grad_norm_(self.actor.parameters(), self.max_grad_norm)
        self.actor_optim.step()
        torch.nn.utils.clip_grad_norm_(self.critic.parameters(), self.max_grad_norm)
        self.critic_optim.step()
        return stats

    # -- the graph --
    def _snapshot(self):
        dev = self._inputs[0].device
        return ([p.detach().clone() for m in (self.actor, self.critic) for p in m.parameters()], self.optim.state_dict(),
                self.actor.step_dropout(dev).state.clone())

    def _restore(self, snap):
        params, optim, drop = snap
        dev = self._inputs[0].device
        with torch.no_grad():
            for p, q in zip([p for m in (self.actor, self.critic) for p in m.parameters()], params):
                p.copy_(q)
            self.optim.load_state_dict(optim)
            self.optim.zero_grad()
            self.actor.step_dropout(dev).state.copy_(drop)

    def capture(self, static, dynamic, decoder_static, decoder_dynamic):
        """Record ``step`` on clones of the four tensors (they fix the shapes) into ONE graph.  A warm-up iteration runs first on a
        side stream, as capture needs, and is undone: parameters, moments, counters and the actor's episode counter
        are put back, so the first ``replay`` is the first iteration.  -> self."""
        if self.tail != 'hip':
            raise RuntimeError("capture() needs the device tail: stock Adam.step() reads on the host")
        if pack._binary_mode != 'trust':
            raise RuntimeError("capture() needs pack.set_binary_check('trust'): the 0/1 check of `dynamic` is a host read")
        if not _on_device(static, dynamic) or not self.optim.on_device:
            raise RuntimeError("capture() needs float32 tensors and modules on the GPU")
        self._inputs = [t.detach().clone() for t in (static, dynamic, decoder_static, decoder_dynamic)]
        dev = static.device
        snap = self._snapshot()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self.step(*self._inputs)
        torch.cuda.current_stream(dev).wait_stream(side)
        self._restore(snap)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._stats = self.step(*self._inputs)
        self._graph = graph
        return self

    def replay(self, static, dynamic, decoder_static, decoder_dynamic):
        """copy a batch of the captured shapes into the graph's input buffers and replay it -> the stats row (the graph's own
        buffer: the next replay overwrites it)"""
        if self._graph is None:
            raise RuntimeError("replay() before capture()")
        for dst, src in zip(self._inputs, (static, dynamic, decoder_static, decoder_dynamic)):
            if dst.shape != src.shape:
                raise ValueError("the graph was captured for %s, got %s" % (tuple(dst.shape), tuple(src.shape)))
            dst.copy_(src, non_blocking=True)
        self._graph.replay()
        return self._stats

    def captured_for(self, static):
        return self._graph is not None and self._inputs[0].shape == static.shape


# ---- the reference's two functions -----------------------------------------------------------------------------------------
def validate(data_loader, actor, save_dir, **kwargs):
    """trainer.py:96-135: the actor in ``eval()`` under ``no_grad`` over the loader -> the mean of the batches' mean rewards;
    ``render_fn`` is called per batch as the reference calls it; the actor is back in ``train()`` on return."""
    actor.eval()
    render_fn = kwargs.get('render_fn')
    if render_fn is not None and not os.path.exists(save_dir):
        os.makedirs(save_dir)
    rewards = []
    for batch_idx, batch in enumerate(data_loader):
        static, dynamic, decoder_static, decoder_dynamic = batch
        if kwargs.get('use_cuda'):
            static, dynamic, decoder_static, decoder_dynamic = (t.cuda() for t in (static, dynamic, decoder_static, decoder_dynamic))
        decoder_input = decoder_static if kwargs['decoder_input_type'] == 'shape_only' else [decoder_static, decoder_dynamic]
        with torch.no_grad():
            start = time.time()
            tour_indices, tour_logp, pack_logp, reward = actor(static, dynamic, decoder_input)
            valid_time = time.time() - start
        reward = reward.mean().item()
        rewards.append(reward)
        if render_fn is not None:
            path = os.path.join(save_dir, 'batch%d_%2.4f.png' % (batch_idx, reward))
            render_fn(static, tour_indices, path, dynamic, valid_time, **kwargs)
    actor.train()
    return np.mean(rewards)


def _plot(save_dir, my_rewards):
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        return
    plt.close('all')
    plt.title('Reward')
    plt.plot(range(len(my_rewards)), my_rewards, '-')
    plt.savefig(save_dir + '/reward.png', bbox_inches='tight', dpi=400)


def train(actor, critic, **kwargs):
    """trainer.py:137-313 with the reference's keyword names and directory layout: ``pack/<num_nodes>/<obj_dim>d-<input_type>-
    <reward_type>-<packing_strategy>-width-<container_width>-note-<note>-<date>/`` holds ``checkpoints/<epoch>/{actor,critic}.pt``,
    the best pair at its top, ``render/<epoch>/``, ``reawrds.txt`` (the reference's spelling), ``losses.txt`` and -- where
    matplotlib imports -- ``reward.png``; the printed lines are the reference's.  An iteration is ``TrainStep.step``; its
    stats stay on the device and are read once per ``log_step`` window, and a window with a flagged env (a placement above
    the container: the reference's IndexError) raises ``TapOverflowError`` there.  ``graph=True`` replays the iteration from
    a graph for every batch of the full batch size (``pack.set_binary_check('trust')`` is set for the run); ``tail``:
    ``TrainStep``'s.  -> the directory."""
    date = datetime.datetime.now()
    now = '%s-%s-%s' % (date.date(), date.hour, date.minute)
    save_dir = os.path.join('pack', '%d' % kwargs['num_nodes'],
                            '%sd-%s-%s-%s-width-%s-note-%s-%s' % (kwargs['obj_dim'], kwargs['input_type'], kwargs['reward_type'],
                                                                  kwargs['packing_strategy'], kwargs['container_width'], kwargs['note'], now))
    checkpoint_dir = os.path.join(save_dir, 'checkpoints')
    os.makedirs(checkpoint_dir, exist_ok=True)
    use_graph = kwargs.get('graph', DEFAULT_GRAPH) and kwargs.get('use_cuda')
    trainer = TrainStep(actor, critic, kwargs['actor_lr'], kwargs['critic_lr'], kwargs['max_grad_norm'], kwargs['obj_dim'],
                        kwargs['decoder_input_type'], tail='hip' if use_graph else kwargs.get('tail'))
    train_loader = DataLoader(kwargs['train_data'], kwargs['batch_size'], shuffle=True, num_workers=0)
    valid_loader = DataLoader(kwargs['valid_data'], len(kwargs['valid_data']), shuffle=False, num_workers=0)
    best_reward = np.inf
    my_rewards, my_losses = [], []
    log_step = min(max(int(kwargs['train_size'] / kwargs['batch_size']), 1), 100)
    binary_mode = pack._binary_mode
    if use_graph:
        pack.set_binary_check('trust')
    try:
        for epoch in range(kwargs['epoch_num']):
            actor.train()
            critic.train()
            times, rows, window = [], [], []
            epoch_start = start = time.time()
            valid_dir = os.path.join(save_dir, 'render', '%s' % epoch)
            os.makedirs(valid_dir, exist_ok=True)

            def read(batch_idx):
                got = torch.stack(window).cpu().numpy().astype(np.float64)      # the ONE host read of the window
                del window[:]
                if got[:, 4].sum() != 0:
                    raise _lib.TapOverflowError(_lib.TAP_E_OVERFLOW, "%d env(s) of the batches up to %d of epoch %d were flagged (a "
                                                "placement above the container height)" % (int(got[:, 4].sum()), batch_idx, epoch))
                rows.extend(got)

            for batch_idx, batch in enumerate(train_loader):
                if kwargs['task'] == 'test':
                    break
                if kwargs['use_cuda']:
                    batch = [t.cuda().detach() for t in batch]
                if use_graph and int(batch[0].shape[0]) == kwargs['batch_size']:
                    if not trainer.captured_for(batch[0]):
                        trainer.capture(*batch)
                    window.append(trainer.replay(*batch).clone())
                else:
                    window.append(trainer.step(*batch))
                if (batch_idx + 1) % log_step == 0:
                    read(batch_idx)
                    end = time.time()
                    times.append(end - start)
                    start = end
                    mean_loss = np.mean([r[0] for r in rows[-log_step:]])
                    mean_reward = np.mean([r[2] for r in rows[-log_step:]])
                    my_rewards.append(mean_reward)
                    my_losses.append(mean_loss)
                    print('    Epoch %d  Batch %d/%d, reward: %2.3f, loss: %2.4f, took: %2.4fs' %
                          (epoch, batch_idx, len(train_loader), mean_reward, mean_loss, times[-1]))
            if window:
                read(len(train_loader) - 1)
            mean_loss = np.mean([r[0] for r in rows])
            mean_reward = np.mean([r[2] for r in rows])
            epoch_dir = os.path.join(checkpoint_dir, '%s' % epoch)
            os.makedirs(epoch_dir, exist_ok=True)
            torch.save(actor.state_dict(), os.path.join(epoch_dir, 'actor.pt'))
            torch.save(critic.state_dict(), os.path.join(epoch_dir, 'critic.pt'))
            mean_valid = validate(valid_loader, actor, valid_dir, **kwargs)
            if mean_valid < best_reward:
                best_reward = mean_valid
                torch.save(actor.state_dict(), os.path.join(save_dir, 'actor.pt'))
                torch.save(critic.state_dict(), os.path.join(save_dir, 'critic.pt'))
            # (the reference hands mean_loss to the 'valid' field and mean_valid to 'loss': its line, kept)
            print('Epoch %d,  mean epoch reward: %2.4f    valid: %2.4f, loss: %2.4f, took: %2.4fs '
                  '(%2.4fs / %d batches)' % (epoch, mean_reward, mean_loss, mean_valid, time.time() - epoch_start, np.mean(times), log_step))
            _plot(save_dir, my_rewards)
            if use_graph:
                pack.check_binary()                               # the deferred 0/1 test of this epoch's `dynamic` tensors
    finally:
        pack.set_binary_check(binary_mode)
    np.savetxt(save_dir + '/reawrds.txt', my_rewards)
    np.savetxt(save_dir + '/losses.txt', my_losses)
    _plot(save_dir, my_rewards)
    return save_dir
