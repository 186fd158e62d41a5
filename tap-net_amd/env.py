"""Batched counterpart of the reference's ``tools.Container`` (tools.py:3607-3966).

``BatchedContainer`` steps B containers in lock-step on one MI355X through libtapenv's HIP
kernels; ``Container`` is the per-env facade with the reference's own method surface
(``add_new_block`` / ``get_heightmap`` / ``calc_ratio`` / ``clear_container`` and the attributes
rolling.py reads), implemented as a BatchedContainer of one.  Neither has a CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


class BatchedContainer(object):
    """B target containers: height-maps + counters in HBM, stepped by one kernel launch.

    Constructor arguments after ``batch_size`` are those of tools.Container.__init__
    (tools.py:3611-3612); ``initial_container_size`` / ``max_height`` are accepted and stored only
    (the reference uses them for drawing).
    """

    def __init__(self, batch_size, container_size, blocks_num, reward_type, heightmap_type='full',
                 initial_container_size=None, max_height=None, packing_strategy='LB_GREEDY',
                 device='cuda', place_at=None):
        self.device = _lib.resolve_device(device)
        self.batch_size = int(batch_size)
        self.container_size = [int(v) for v in container_size]
        self.block_dim = len(self.container_size)
        self.blocks_num = int(blocks_num)
        self.reward_type = reward_type
        self.heightmap_type = heightmap_type
        self.initial_container_size = initial_container_size
        self.max_height = 2 * self.container_size[0] if max_height is None else max_height  # tools.py:3624-3627
        self.desc = _lib.make_desc(self.batch_size, self.container_size, blocks_num, reward_type,
                                   heightmap_type, packing_strategy)
        # the pack-net placement (tapenv.h: tap_env_step_at): blocks at caller-chosen columns, stepped by
        # add_new_blocks_at* only; 'container' = tools.Container.add_new_block_at, 'net' = tools.calc_one_position_net
        self.place_at = place_at
        if place_at is not None:
            _lib.set_place_at(self.desc, place_at)
        # tools.py:3617-3620: the reward string may override the strategy
        if reward_type in ('C+P+S-mul-soft', 'C+P+S-mul-hard'):
            packing_strategy = 'MUL'
        elif reward_type in ('C+P+S-mcs-soft', 'C+P+S-mcs-hard'):
            packing_strategy = 'MACS'
        self.packing_strategy = packing_strategy
        self._ctx = _lib.ctx(self.device)
        nbytes = _lib.lib().tap_env_state_bytes(C.byref(self.desc))
        self._state = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        self._flen = _lib.lib().tap_env_feature_len(C.byref(self.desc))
        self.reset()

    @property
    def fused_ok(self):
        """False for the shapes / strategies whose step is not ONE kernel: the legacy 'LB' strategy, LB_GREEDY
        and MACS 3D containers above 64 cells or with a 3D side above 8 (one wavefront -- legacy 'LB': one thread -- per container, lb.hip / big.hip /
        macs3_big.hip) and MACS 2D
        containers above 16 columns (a single kernel was measured slower than the two launches there).
        tap_transition* / tap_rolling_step take them all the same and run the two launches themselves."""
        d = self.desc
        over = d.W * d.L > 64 or (d.D == 3 and (d.W > 8 or d.L > 8))
        big = over and (d.strategy == _lib.TAP_LB_GREEDY or (d.strategy == _lib.TAP_MACS and d.D == 3))   # big.hip / macs3_big.hip
        wide_macs = d.strategy == _lib.TAP_MACS and d.D == 2 and d.W > 16           # above 16 columns: one wavefront per container
        return not (big or wide_macs or d.strategy == _lib.TAP_LB)

    # ---- plumbing ---------------------------------------------------------------------------
    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            _lib.check(fn(self._ctx, C.byref(self.desc), *args, _lib.stream_of(self.device)), self._ctx)

    def _feature_shape(self):
        d = self.desc
        if d.D == 2:
            return (self.batch_size, self._flen, 1)              # model.py:456-458 .unsqueeze(2)
        if self.heightmap_type == 'diff':
            return (self.batch_size, 2, d.W, d.L)                # model.py:461-463
        return (self.batch_size, 1, d.W, d.L)                    # model.py:464-465 .unsqueeze(1)

    def _new_feature(self):
        return torch.empty(self._feature_shape(), dtype=torch.float32, device=self.device)

    def _as_active(self, active):
        if active is None:
            return None
        a = torch.as_tensor(active, device=self.device)
        if a.numel() != self.batch_size:
            raise ValueError("active must have %d entries, got %s" % (self.batch_size, tuple(a.shape)))
        return a.to(torch.uint8).contiguous()

    # ---- tools.Container surface, batched ---------------------------------------------------
    def reset(self):
        """clear_container for every env (tools.py:3858-3885)."""
        self._call(_lib.lib().tap_env_reset, _lib.ptr(self._state))

    clear_container = reset

    def add_new_blocks(self, blocks, active=None, want_feature=True):
        """add_new_block for all envs (tools.py:3663-3744): ``blocks`` (B, D) float32/int32 tensor
        (or anything torch.as_tensor accepts).  Returns the heightmap feature in the layout
        model.py:456-465 feeds the decoder, or None if ``want_feature`` is False."""
        blocks = torch.as_tensor(blocks, device=self.device)
        if blocks.dim() == 3 and blocks.shape[-1] == 1:          # decoder_static (B, D, 1), model.py:404-412
            blocks = blocks.squeeze(-1)
        if tuple(blocks.shape) != (self.batch_size, self.block_dim):
            raise ValueError("blocks must be (%d, %d), got %s" % (self.batch_size, self.block_dim, tuple(blocks.shape)))
        if blocks.dtype == torch.int32:
            dt = _lib.TAP_DT_I32
        else:
            blocks = blocks.to(torch.float32)
            dt = _lib.TAP_DT_F32
        blocks = blocks.contiguous()
        act = self._as_active(active)
        feat = self._new_feature() if want_feature else None
        self._call(_lib.lib().tap_env_step, _lib.ptr(self._state), _lib.ptr(blocks), dt,
                   _lib.ptr(act), _lib.ptr(feat))
        return feat

    def add_new_blocks_gather(self, static, ptr, active=None, want_feature=True, out=None):
        """Same, with the gather of model.py:404-412 fused: block = static[b, 1:1+D, ptr[b]]."""
        if static.dtype != torch.float32 or not static.is_contiguous() or static.device != self.device:
            static = static.to(device=self.device, dtype=torch.float32).contiguous()
        ptr = ptr.to(device=self.device, dtype=torch.int64).contiguous()
        if static.dim() != 3 or static.shape[0] != self.batch_size or static.shape[1] < 1 + self.block_dim:
            raise ValueError("static must be (%d, >= %d, nR), got %s" % (self.batch_size, 1 + self.block_dim, tuple(static.shape)))
        if tuple(ptr.shape) != (self.batch_size,):
            raise ValueError("ptr must be (%d,), got %s" % (self.batch_size, tuple(ptr.shape)))
        act = self._as_active(active)
        feat = out if out is not None else (self._new_feature() if want_feature else None)
        if feat is not None and (tuple(feat.shape) != self._feature_shape() or feat.dtype != torch.float32 or not feat.is_contiguous()):
            raise ValueError("out must be a contiguous float32 tensor of shape %s" % (self._feature_shape(),))
        self._call(_lib.lib().tap_env_step_gather, _lib.ptr(self._state), _lib.ptr(static),
                   static.shape[1], static.shape[2], _lib.ptr(ptr), _lib.ptr(act), _lib.ptr(feat))
        return feat

    def trial_scores(self, static, mask=None, fresh=False, out=None, best_out=None, stepped=False):
        """What would calc_ratio be if env b took column c next -- for every selectable column, nothing committed
        (tapenv.h: tap_env_trial_scores; the reference's best_to_pack, generate.py:1242-1292).  ``static`` (B, >= 1+D,
        nR) float32; ``mask`` (B, nR) float32 or None = every column (the stepper's ``current_mask``); ``fresh``: score
        against a freshly reset container whatever the blob holds.  -> (scores (B, nR) float64, best (B,) int64):
        the fp64 calc_ratio after the step for a selectable column, -1.0 where that step would raise an error bit, -inf
        for an unselectable one; ``best`` the first column with the row's maximum (0 where none is selectable).  The
        state blob is only read.  ``out`` / ``best_out``: buffers to fill -- with both given nothing is allocated and the
        call is one launch (capturable in a hipGraph).  The one-launch kernel takes the lane-per-cell LB_GREEDY shapes;
        for every other strategy and size the step entry points take (TAP_E_UNSUPPORTED), or with ``stepped=True``,
        the same answer comes from nR committed steps on a scratch copy of the blob (_trial_scores_stepped)."""
        if static.dtype != torch.float32 or not static.is_contiguous() or static.device != self.device:
            static = static.to(device=self.device, dtype=torch.float32).contiguous()
        if static.dim() != 3 or static.shape[0] != self.batch_size or static.shape[1] < 1 + self.block_dim:
            raise ValueError("static must be (%d, >= %d, nR), got %s" % (self.batch_size, 1 + self.block_dim, tuple(static.shape)))
        B, nR = self.batch_size, int(static.shape[2])
        if mask is not None:
            if tuple(mask.shape) != (B, nR):
                raise ValueError("mask must be (%d, %d), got %s" % (B, nR, tuple(mask.shape)))
            if mask.dtype != torch.float32 or not mask.is_contiguous() or mask.device != self.device:
                mask = mask.to(device=self.device, dtype=torch.float32).contiguous()
        for t, shape, dt, what in ((out, (B, nR), torch.float64, "out"), (best_out, (B,), torch.int64, "best_out")):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device):
                raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (what, dt, shape, self.device))
        scores = out if out is not None else torch.empty(B, nR, dtype=torch.float64, device=self.device)
        best = best_out if best_out is not None else torch.empty(B, dtype=torch.int64, device=self.device)
        if self.place_at is not None and stepped:
            raise _lib.TapError(_lib.TAP_E_INVALID, "trial scores on a place-at container: its blocks go to caller-chosen columns")
        if not stepped:
            try:
                self._call(_lib.lib().tap_env_trial_scores, _lib.ptr(self._state), _lib.ptr(static), static.shape[1], nR,
                           _lib.ptr(mask), _lib.TAP_T_FRESH if fresh else 0, _lib.ptr(scores), _lib.ptr(best))
                return scores, best
            except _lib.TapError as e:
                if e.status != _lib.TAP_E_UNSUPPORTED:
                    raise
        return self._trial_scores_stepped(static, mask, fresh, scores, best)

    def _trial_scores_stepped(self, static, mask, fresh, scores, best):
        """trial_scores from the kernels every strategy and size has: per column, a scratch blob takes a copy of the
        state (a reset under ``fresh``), one committed tap_env_step_gather with that column for every env, then
        tap_env_ratio in fp64 and the error words; the same -inf / -1.0 / first-maximum rules on top."""
        B, nR = self.batch_size, int(static.shape[2])
        if getattr(self, "_trial_state", None) is None:
            self._trial_state = torch.empty_like(self._state)
        scratch, L = self._trial_state, _lib.lib()
        # the blob's error words: its third section, after the height-maps and the counters (each 256-byte aligned)
        al = lambda v: (v + 255) & ~255  # noqa: E731
        off = al(B * self.desc.W * self.desc.L * 4) + al(B * 16)
        scratch_err = scratch[off:off + 4 * B].view(torch.int32)
        ptr = torch.empty(B, dtype=torch.int64, device=self.device)
        r64 = torch.empty(B, dtype=torch.float64, device=self.device)
        err = torch.empty(B, dtype=torch.int32, device=self.device)
        for c in range(nR):
            if fresh:
                self._call(L.tap_env_reset, _lib.ptr(scratch))
            else:
                scratch.copy_(self._state)
                scratch_err.zero_()                            # the trial's own error bits, not the blob's sticky ones
            ptr.fill_(c)
            self._call(L.tap_env_step_gather, _lib.ptr(scratch), _lib.ptr(static), static.shape[1], nR, _lib.ptr(ptr),
                       None, None)
            self._call(L.tap_env_ratio, _lib.ptr(scratch), None, _lib.ptr(r64), None)
            self._call(L.tap_env_errors, _lib.ptr(scratch), _lib.ptr(err))
            scores[:, c] = torch.where(err != 0, torch.full_like(r64, -1.0), r64)
        if mask is not None:
            scores.masked_fill_(mask == 0, float('-inf'))
        # the first column holding the maximum; a NaN score (0 / 0: a block that fits nowhere in an empty container)
        # is never the best
        key = torch.where(torch.isnan(scores), torch.full_like(scores, float('-inf')), scores)
        cols = torch.arange(nR, device=self.device).expand(B, nR)
        at_max = key == key.max(dim=1, keepdim=True).values
        best.copy_(torch.where(at_max, cols, torch.full_like(cols, nR)).min(dim=1).values)
        return scores, best

    def _pnet_args(self, pnet_out, pnet_form):
        if pnet_out is None:
            return None, 0
        if self.place_at is None:
            raise ValueError("pnet_out is written by the place-at step only")
        d = self.desc
        if tuple(pnet_out.shape) != (self.batch_size, 1, d.W) or pnet_out.dtype != torch.float32 \
                or not pnet_out.is_contiguous() or pnet_out.device != self.device:
            raise ValueError("pnet_out must be a contiguous float32 tensor of shape (%d, 1, %d) on %s"
                             % (self.batch_size, d.W, self.device))
        if pnet_form is None:                    # calc_positions_net feeds the raw map (tools.py:3407), DRL_L its own form
            pnet_form = 'full' if self.place_at == 'net' else self.heightmap_type
        if pnet_form not in _lib.PNET_FORMS:
            raise ValueError("pnet_form must be 'full', 'zero' or 'diff', not %r" % (pnet_form,))
        return pnet_out, _lib.PNET_FORMS[pnet_form]

    def _as_pos_x(self, pos_x):
        x = torch.as_tensor(pos_x, device=self.device)
        if x.numel() != self.batch_size:
            raise ValueError("pos_x must have %d entries, got %s" % (self.batch_size, tuple(x.shape)))
        return x.reshape(-1).to(torch.int64).contiguous()

    def add_new_blocks_at(self, blocks, pos_x, active=None, want_feature=True, pnet_out=None, pnet_form=None):
        """add_new_block_at for all envs (tools.py:3746-3822; with place_at='net' calc_one_position_net's placement,
        tools.py:3371-3461): ``blocks`` (B, 2) float32/int32, ``pos_x`` (B,) column indices.  Returns the decoder
        feature as add_new_blocks does.  ``pnet_out`` (B, 1, W) float32, optional: filled with the pack-net's input
        for the next step, in form ``pnet_form`` ('full' / 'zero' / 'diff' in DRL_L's length-W form, model.py:1173-1196;
        default 'full' for place_at='net', heightmap_type for 'container').  One launch."""
        blocks = torch.as_tensor(blocks, device=self.device)
        if blocks.dim() == 3 and blocks.shape[-1] == 1:
            blocks = blocks.squeeze(-1)
        if tuple(blocks.shape) != (self.batch_size, self.block_dim):
            raise ValueError("blocks must be (%d, %d), got %s" % (self.batch_size, self.block_dim, tuple(blocks.shape)))
        if blocks.dtype == torch.int32:
            dt = _lib.TAP_DT_I32
        else:
            blocks = blocks.to(torch.float32)
            dt = _lib.TAP_DT_F32
        blocks = blocks.contiguous()
        x = self._as_pos_x(pos_x)
        po, pf = self._pnet_args(pnet_out, pnet_form)
        act = self._as_active(active)
        feat = self._new_feature() if want_feature else None
        self._call(_lib.lib().tap_env_step_at, _lib.ptr(self._state), _lib.ptr(blocks), dt, _lib.ptr(act),
                   _lib.ptr(feat), _lib.ptr(x), _lib.ptr(po), pf)
        return feat

    def add_new_blocks_at_gather(self, static, ptr, pos_x, active=None, want_feature=True, out=None, pnet_out=None,
                                 pnet_form=None):
        """Same, with the gather of model.py:1164-1167 fused: block = static[b, 1:3, ptr[b]]."""
        if static.dtype != torch.float32 or not static.is_contiguous() or static.device != self.device:
            static = static.to(device=self.device, dtype=torch.float32).contiguous()
        ptr = ptr.to(device=self.device, dtype=torch.int64).contiguous()
        if static.dim() != 3 or static.shape[0] != self.batch_size or static.shape[1] < 1 + self.block_dim:
            raise ValueError("static must be (%d, >= %d, nR), got %s" % (self.batch_size, 1 + self.block_dim, tuple(static.shape)))
        if tuple(ptr.shape) != (self.batch_size,):
            raise ValueError("ptr must be (%d,), got %s" % (self.batch_size, tuple(ptr.shape)))
        x = self._as_pos_x(pos_x)
        po, pf = self._pnet_args(pnet_out, pnet_form)
        act = self._as_active(active)
        feat = out if out is not None else (self._new_feature() if want_feature else None)
        if feat is not None and (tuple(feat.shape) != self._feature_shape() or feat.dtype != torch.float32 or not feat.is_contiguous()):
            raise ValueError("out must be a contiguous float32 tensor of shape %s" % (self._feature_shape(),))
        self._call(_lib.lib().tap_env_step_at_gather, _lib.ptr(self._state), _lib.ptr(static), static.shape[1],
                   static.shape[2], _lib.ptr(ptr), _lib.ptr(act), _lib.ptr(feat), _lib.ptr(x), _lib.ptr(po), pf)
        return feat

    def get_heightmaps(self):
        """get_heightmap for all envs (tools.py:3824-3856), same layout as add_new_blocks."""
        feat = self._new_feature()
        self._call(_lib.lib().tap_env_feature, _lib.ptr(self._state), _lib.ptr(feat))
        return feat

    def calc_ratios(self, out=None):
        """calc_ratio for all envs as the fp32 tensor model.py:499-510 builds."""
        r = out if out is not None else torch.empty(self.batch_size, dtype=torch.float32, device=self.device)
        self._call(_lib.lib().tap_env_ratio, _lib.ptr(self._state), _lib.ptr(r), None, None)
        return r

    def calc_ratios64(self):
        r = torch.empty(self.batch_size, dtype=torch.float64, device=self.device)
        self._call(_lib.lib().tap_env_ratio, _lib.ptr(self._state), None, _lib.ptr(r), None)
        return r

    def calc_CPS(self):
        """(B, 3) float64 tensor of C, P, S (tools.py:3887-3905)."""
        cps = torch.empty(self.batch_size, 3, dtype=torch.float64, device=self.device)
        self._call(_lib.lib().tap_env_ratio, _lib.ptr(self._state), None, None, _lib.ptr(cps))
        return cps

    @property
    def errors(self):
        """(B,) int32 sticky error words (tapenv.h: tap_env_errors), asynchronously: bit 1 = a placement reached above
        the container height, 2 = too many steps, 4 = bad block / column index, 8 / 16 = MACS list guards."""
        err = torch.empty(self.batch_size, dtype=torch.int32, device=self.device)
        self._call(_lib.lib().tap_env_errors, _lib.ptr(self._state), _lib.ptr(err))
        return err

    def check(self):
        """Synchronises; raises TapOverflowError (an IndexError, like the reference) if any env
        was pushed above its height, TapError for other sticky errors."""
        n_bad = C.c_int32(0)
        with torch.cuda.device(self.device):
            st = _lib.lib().tap_env_check(self._ctx, C.byref(self.desc), _lib.ptr(self._state),
                                          C.byref(n_bad), _lib.stream_of(self.device))
        _lib.check(st, self._ctx)

    # ---- attributes -------------------------------------------------------------------------
    def _export(self, hm=False, pos=False, st=False, cnt=False):
        d, B = self.desc, self.batch_size
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)  # noqa: E731
        o_hm = mk((B, d.W * d.L), torch.int32) if hm else None
        o_pos = mk((B, d.n_max, d.D), torch.int32) if pos else None
        o_st = mk((B, d.n_max), torch.uint8) if st else None
        o_cnt = mk((B, 4), torch.int32) if cnt else None
        self._call(_lib.lib().tap_env_export, _lib.ptr(self._state), _lib.ptr(o_hm), _lib.ptr(o_pos),
                   _lib.ptr(o_st), _lib.ptr(o_cnt))
        return o_hm, o_pos, o_st, o_cnt

    @property
    def heightmap(self):
        hm = self._export(hm=True)[0]
        d = self.desc
        return hm.view(self.batch_size, d.W, d.L) if d.D == 3 else hm

    @property
    def positions(self):
        return self._export(pos=True)[1]

    @property
    def stable(self):
        return self._export(st=True)[2].bool()

    @property
    def counters(self):
        """(B, 4) int32: valid_size, empty_size, sum(stable), current_blocks_num."""
        return self._export(cnt=True)[3]

    @property
    def valid_size(self):
        return self.counters[:, 0]

    @property
    def empty_size(self):
        return self.counters[:, 1]

    @property
    def current_blocks_num(self):
        return self.counters[:, 3]

    def state_dict(self):
        return {'state': self._state.clone(), 'desc': bytes(self.desc)}

    def load_state_dict(self, sd):
        if sd['desc'] != bytes(self.desc):
            raise ValueError("state_dict was saved for a different container description")
        self._state.copy_(sd['state'])


class PackEngines(object):
    """B of the global pack-net's own environments (pack_net/LG_RL.py: PackEngine, LG_RL.py:414-528) in one state blob,
    stepped by one launch per inner step for all of them (tapenv.h: tap_env_step_engine).  ``T`` is the longest block
    sequence a forward hands in (the tape's length); ``max_blocks_num`` the engine's wrap period (PackEngine clears
    after that many steps, LG_RL.py:482-491; 0 = never, the replay of LG_RL.calc_positions).  Nothing is read back to
    the host.

    step(i, blocks, x) places blocks[:, :, i] of a (B, 2, T') float32 array (T' <= T) at columns x (B,) int64 and
    returns the net's next input (B, W', 1) float32 in ``heightmap_type`` form (W' = W - 1 for 'diff'); with
    ``want_reward`` it also refreshes ``reward`` (B,) float32, the step's (C+P+S)/3.  Step 0 -- and every
    i % max_blocks_num == 0 -- starts from the empty container, so a forward needs no reset launch."""

    def __init__(self, batch_size, container_width, container_height, T, heightmap_type='diff', max_blocks_num=10,
                 device='cuda'):
        if heightmap_type not in ('full', 'zero', 'diff'):
            raise ValueError("heightmap_type must be 'full', 'zero' or 'diff', not %r" % (heightmap_type,))
        if int(max_blocks_num) < 0:
            raise ValueError("max_blocks_num must be >= 0")
        self.batch_size, self.W, self.H, self.T = int(batch_size), int(container_width), int(container_height), int(T)
        self.heightmap_type = heightmap_type
        self.max_blocks_num = int(max_blocks_num)
        self.env = BatchedContainer(self.batch_size, [self.W, self.H], self.T, 'C+P+S-G-soft', heightmap_type,
                                    device=device, place_at='net')
        self.device = self.env.device
        self.reward = torch.zeros(self.batch_size, dtype=torch.float32, device=self.device)
        self.last_input = None                   # what the last step returned: the blob's state in heightmap_type form

    def reset(self):
        """PackEngine.clear for every env (one launch; step 0 of a forward clears by itself)."""
        self.env.reset()
        self.last_input = None

    def _blocks(self, blocks):
        if blocks.dim() != 3 or blocks.shape[0] != self.batch_size or blocks.shape[1] != 2:
            raise ValueError("blocks must be (%d, 2, T), got %s" % (self.batch_size, tuple(blocks.shape)))
        if blocks.dtype != torch.float32 or blocks.device != self.device or not blocks.is_contiguous():
            blocks = blocks.to(device=self.device, dtype=torch.float32).contiguous()
        return blocks

    def step(self, i, blocks, x, want_reward=True, out=None, want_input=True):
        """PackEngine.step of every env at inner step ``i`` (LG_RL.py:440-496): see the class docstring.  Returns None
        with ``want_input=False`` (the replay of LG_RL.calc_positions reads only the counters and the tape)."""
        blocks = self._blocks(blocks)
        Tb = int(blocks.shape[2])
        i = int(i)
        if not 0 <= i < min(Tb, self.T):
            raise ValueError("step %d outside the %d blocks handed in / the tape of %d" % (i, Tb, self.T))
        x = self.env._as_pos_x(x)
        shape = self.env._feature_shape()
        if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous()
                                or out.device != self.device):
            raise ValueError("out must be a contiguous float32 tensor of shape %s on %s" % (shape, self.device))
        feat = out if out is not None else (self.env._new_feature() if want_input else None)
        self.env._call(_lib.lib().tap_env_step_engine, _lib.ptr(self.env._state), _lib.ptr(blocks), Tb, i,
                       self.max_blocks_num, _lib.ptr(x), _lib.ptr(feat), _lib.ptr(self.reward if want_reward else None))
        self.last_input = feat
        return feat

    @property
    def positions(self):
        """(B, T, 2) int32: (x after the clamp, z) of every step of the last forward, by step index"""
        return self.env.positions

    @property
    def stable(self):
        """(B, T) bool"""
        return self.env.stable

    @property
    def errors(self):
        return self.env.errors

    def check(self):
        self.env.check()

    def get_heightaps(self, heightmap_type):
        """PackEngine.get_heightap (LG_RL.py:498-515) of every env: (B, W', 1) float32 -- 'full' the height-map, 'zero'
        minus its minimum, 'diff' hm[c+1] - hm[c] (W - 1 entries)."""
        if heightmap_type == self.heightmap_type and self.last_input is not None:
            return self.last_input
        hm = self.env.heightmap.to(torch.float32)
        if heightmap_type == 'full':
            out = hm
        elif heightmap_type == 'zero':
            out = hm - hm.min(dim=1, keepdim=True).values
        elif heightmap_type == 'diff':
            out = hm[:, 1:] - hm[:, :-1]
        else:
            raise ValueError("heightmap_type must be 'full', 'zero' or 'diff', not %r" % (heightmap_type,))
        return out.unsqueeze(2).contiguous()


# ---- lock-step pooling of per-env Containers -------------------------------------------------------------------------
# model.py:294 builds `batch_size` tools.Container objects and model.py:451-453 calls each of them once per decoding
# step before it stacks the results (torch.FloatTensor(heightmaps), model.py:454-465); model.py:509-510 does the same
# with calc_ratio.  With pooling on, the Containers built back to back with the same arguments share ONE
# BatchedContainer: a member's add_new_block / get_heightmap only records its request and hands back ITS ROW of the
# step's result array; the call that completes the round (every member has been called once) runs one launch for the
# whole pool and fills the array in place -- the rows handed out earlier are views of it.  One launch, one host->device
# and one device->host copy per decoding step instead of batch_size of each, with model.py unchanged.
# The contract is model.py's own call pattern: read the rows only after the round's last call.  A member called twice
# within a round, or any attribute / calc_ratio read, completes the round early (the members not yet called just do
# not step), so nothing is ever left un-run -- but a row read before its round completed holds no data.  Off by
# default (every Container is then its own one-env launch + sync, correct for any pattern); switch it on with
# `with tools.lockstep_scope():` around the forward (the pool is closed at the end of the block),
# tools.lockstep_containers(True) or TAP_LOCKSTEP_CONTAINERS=1.
# Membership: the Containers built back to back with the same arguments while the pool is open (it closes at its first
# use, at the end of a lockstep_scope, or at the next lockstep_containers call).  A Container that was collected before
# the pool's first use is not waited for; one that is alive but never called (a probe built with the same arguments
# outside a scope) makes the first "second call" raise LockstepError and is dropped -- rows are handed out holding a
# sentinel (int64 min), never stale memory; the raising call is recorded in the new round first (its row: err.row).  The 'mul' input types pool containers_a and containers_b together
# (model.py:290-292 builds them alternately with the same arguments): every env calls exactly one method on each of
# its two Containers per step (model.py:419-427), so a round is 2 * batch_size calls.
import os as _os

_lockstep = _os.environ.get("TAP_LOCKSTEP_CONTAINERS", "0") not in ("", "0")
_open_pool = None


def lockstep_containers(on=True):
    """Pool the Containers built from now on (see above) -> the previous setting.  Any pool still open is closed:
    Containers built after this call never join a pool started before it."""
    global _lockstep, _open_pool
    prev, _lockstep, _open_pool = _lockstep, bool(on), None
    return prev


class lockstep_scope(object):
    """``with lockstep_scope():`` -- pooling on for the Containers built inside the block, and the pool CLOSED at its
    end, so that a later Container with the same arguments (a probe, a warm-up forward, the next forward) can never
    join it; the previous setting is restored."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        self.prev = lockstep_containers(self.on)
        return self

    def __exit__(self, *exc):
        lockstep_containers(self.prev)
        return False


_draw_warned = False
_UNFILLED = np.iinfo(np.int64).min    # a row handed out before its round completed holds this, never stale data


class LockstepError(RuntimeError):
    """A lock-step round was completed with members that were never called (see _Pool.flush)."""


class _Pool(object):
    def __init__(self, key, args):
        self.key, self.args = key, args
        self.members = 0
        self.refs = []                  # weak references to the member Containers (a collected one leaves the pool)
        self.env = None                 # built when the first member is used: the pool is sealed then
        self.place_at = None            # 'container' once a member called add_new_block_at (Container.add_new_block_at)
        self.stepped = False            # an add_new_block round has run: the pool can no longer switch to place-at
        self.hm_cache = None            # place-at pools: every member's height-map, read once per round (DRL_L, model.py:1176-1178)

    def join(self, owner):
        import weakref
        i = self.members
        self.members += 1
        self.refs.append(weakref.ref(owner))
        return i

    def seal(self):
        global _open_pool
        if self.env is not None:
            return
        if _open_pool is self:
            _open_pool = None
        (cs, n, reward, hm_type, init_cs, max_h, strategy, device) = self.args
        B = self.members
        self.env = BatchedContainer(B, cs, n, reward, hm_type, init_cs, max_h, strategy, device, place_at=self.place_at)
        D = self.env.block_dim
        self.blocks = np.zeros((B, D), np.float32)
        self.pos = [0] * B                                       # place-at columns of this round (ints or 0-d tensors)
        self.active = np.zeros(B, np.uint8)
        self.called = np.zeros(B, bool)
        self.ever = np.zeros(B, bool)                            # called in any round so far
        # members whose Container was already collected when the pool is first used (an abandoned forward) are not
        # waited for; the others are expected once per round
        self.live = np.array([r() is not None for r in self.refs], bool)
        self.n_called = 0
        self.out = None                                          # this round's result rows
        self.ratios = None
        self._fshape = tuple(self.env._feature_shape()[1:])
        if D == 2:
            self._fshape = self._fshape[:1]                      # (W-1,) / (W,): the facade returns the 1-D map
        elif hm_type != 'diff':
            self._fshape = self._fshape[1:]                      # (W, L)

    def use_place_at(self):
        """the first add_new_block_at of a member: from now on the pool steps with tap_env_step_at (CONTAINER semantics).
        A pool whose env was built unflagged (a height-map read before the first step) is rebuilt; one that has run
        add_new_block rounds cannot switch."""
        if self.place_at == 'container':
            return
        if self.env is not None:
            self.flush()
        if self.stepped:
            raise NotImplementedError("add_new_block_at on a lock-step pool whose Containers were stepped with "
                                      "add_new_block: one Container uses one of the two placements, not both")
        self.place_at = 'container'
        if self.env is not None:
            (cs, n, reward, hm_type, init_cs, max_h, strategy, device) = self.args
            self.env = BatchedContainer(self.members, cs, n, reward, hm_type, init_cs, max_h, strategy, device,
                                        place_at=self.place_at)
            self.hm_cache = None

    def heightmap(self, i):
        """member i's height-map; a place-at pool reads every member's once per round"""
        self.seal()
        self.flush()
        if self.hm_cache is None:
            self.hm_cache = self.env.heightmap.cpu().numpy().astype(np.int64)
        return self.hm_cache[i].copy()

    def request(self, i, block, pos_x=None):
        """member i's call of this round: block = None for get_heightmap (report only); pos_x: add_new_block_at's column"""
        self.seal()
        if self.called[i]:
            # a second call within a round: the caller believes the round is over.  Members that were never called
            # in ANY round are phantoms (a probe or warm-up Container built with the same arguments): the rows handed
            # out this round were only filled now, after the caller may have stacked them -- say so instead of
            # letting uninitialised features through, and stop waiting for the phantoms
            phantom = self.live & ~self.ever & ~self.called
            self.flush()
            if phantom.any():
                self.live &= ~phantom
                # the call that found the phantoms is the first call of the NEXT round: it is recorded there before the
                # error leaves (a caller that catches the error and goes on must not end up with this container one
                # step behind the others); its result row rides on the exception
                err = LockstepError(
                    "%d of the %d Containers of this lock-step pool were never called: the round could not complete on "
                    "its last call and its rows were filled late.  Build the pooled Containers inside "
                    "`with tools.lockstep_scope():` (or call tools.lockstep_containers(True) right before model.py:294 "
                    "builds them) so that no other Container with the same arguments joins the pool.  The phantom "
                    "members have been dropped and the next rounds are complete; THIS call was recorded as the first of "
                    "the next round -- do not re-issue it, its result row is the exception's `.row` (filled when that "
                    "round completes)." % (int(phantom.sum()), self.members))
                err.row = self._record(i, block, pos_x)
                raise err
        return self._record(i, block, pos_x)

    def _record(self, i, block, pos_x=None):
        if self.out is None:
            self.out = np.full((self.members,) + self._fshape, _UNFILLED, np.int64)
        if block is not None:
            self.blocks[i] = block
            self.active[i] = 1
            if self.place_at is not None:
                self.pos[i] = pos_x
        self.called[i] = True
        self.ever[i] = True
        self.live[i] = True
        self.n_called += 1
        row = self.out[i]
        if self.n_called >= int(self.live.sum()) and bool(self.called[self.live].all()):
            self.flush()
        return row

    def flush(self):
        if self.env is None or self.n_called == 0:
            return
        env = self.env
        out = self.out
        # the round's bookkeeping is reset BEFORE anything that can raise: an error in one member (TapOverflowError
        # from check()) must not leave `called` set and replay the same blocks on the next request
        blocks, active = torch.from_numpy(self.blocks.copy()), torch.from_numpy(self.active.copy())
        self.active[:] = 0
        self.called[:] = False
        self.n_called = 0
        self.out = None
        self.ratios = None
        self.hm_cache = None
        if self.place_at is not None:
            pos, self.pos = self.pos, [0] * self.members
            feat = env.add_new_blocks_at(blocks, self._columns(pos), active=active)
        else:
            self.stepped = self.stepped or bool(active.any())
            feat = env.add_new_blocks(blocks, active=active)
        out[...] = feat.detach().cpu().numpy().reshape(out.shape)
        env.check()

    def _columns(self, pos):
        """the round's columns as one (B,) int64 device tensor: DRL_L hands each member a 0-d element of its argmax
        tensor (model.py:1200, 1211), stacked here in one op -- no host read per member"""
        dev = self.env.device
        if all(isinstance(v, torch.Tensor) for v in pos):
            return torch.stack([v.reshape(()).to(device=dev, dtype=torch.int64) for v in pos])
        if not any(isinstance(v, torch.Tensor) for v in pos):
            return torch.as_tensor(np.asarray(pos, dtype=np.int64), device=dev)
        return torch.stack([torch.as_tensor(v, device=dev).reshape(()).to(torch.int64) for v in pos])

    def ratio(self, i):
        self.seal()
        self.flush()
        if self.ratios is None:
            self.ratios = self.env.calc_ratios64().cpu().numpy()
        return float(self.ratios[i])


class Container(object):
    """Drop-in for ``tools.Container`` (tools.py:3607): one container, numpy in / numpy out, the
    placement computed by the same HIP kernels -- a BatchedContainer of its own (one launch and one sync per call),
    or, with ``lockstep_containers(True)``, one row of the BatchedContainer it shares with the Containers built
    beside it (one launch per decoding step for all of them, see above)."""

    def __init__(self, container_size, blocks_num, reward_type, heightmap_type='full',
                 initial_container_size=None, max_height=None, packing_strategy='LB_GREEDY',
                 device='cuda'):
        global _open_pool
        self._pool = self._b = None
        self._mode = None                   # 'block' after add_new_block, 'at' after add_new_block_at (one or the other)
        self._args = (container_size, blocks_num, reward_type, heightmap_type, initial_container_size, max_height,
                      packing_strategy, device)
        if _lockstep:
            key = (tuple(int(v) for v in container_size), int(blocks_num), reward_type, heightmap_type,
                   None if initial_container_size is None else tuple(initial_container_size), max_height, packing_strategy,
                   str(device))
            if _open_pool is None or _open_pool.key != key or _open_pool.env is not None:
                _open_pool = _Pool(key, (list(container_size), blocks_num, reward_type, heightmap_type, initial_container_size,
                                         max_height, packing_strategy, device))
            self._pool = _open_pool
            self._i = self._pool.join(self)
            strategy = packing_strategy
            if reward_type in ('C+P+S-mul-soft', 'C+P+S-mul-hard'):          # tools.py:3617-3620
                strategy = 'MUL'
            elif reward_type in ('C+P+S-mcs-soft', 'C+P+S-mcs-hard'):
                strategy = 'MACS'
            self.packing_strategy = strategy
            self.max_height = 2 * int(container_size[0]) if max_height is None else max_height
            self.block_dim = len(container_size)
        else:
            self._b = BatchedContainer(1, container_size, blocks_num, reward_type, heightmap_type,
                                       initial_container_size, max_height, packing_strategy, device)
            self._i = 0
            self.block_dim = self._b.block_dim
            self.packing_strategy = self._b.packing_strategy
            self.max_height = self._b.max_height
        self.reward_type = reward_type
        self.blocks_num = int(blocks_num)
        self.container_size = container_size
        self.initial_container_size = initial_container_size
        self.heightmap_type = heightmap_type
        self.blocks = []
        self.rotate_state = [False] * self.blocks_num
        self.bounding_box = np.zeros(self.block_dim)

    @property
    def _env(self):
        """the BatchedContainer holding this container (a pool's pending round is completed first)"""
        if self._pool is not None:
            self._pool.seal()
            self._pool.flush()
            return self._pool.env
        return self._b

    def _shape(self, feat):
        a = feat.detach().cpu().numpy().astype(np.int64)
        if self.block_dim == 2:
            return a.reshape(-1)
        return a.reshape(a.shape[1:]) if self.heightmap_type == 'diff' else a.reshape(a.shape[2:])

    def add_new_block(self, block, is_rotate=False):
        if self._mode == 'at' or (self._pool is not None and self._pool.place_at is not None):
            raise NotImplementedError("add_new_block on a Container stepped with add_new_block_at: this package runs "
                                      "one of the two placements per Container (and per lock-step pool), not both")
        n = len(self.blocks)
        if n >= self.blocks_num:
            raise IndexError("list assignment index out of range")   # tools.py:3677
        self._mode = 'block'
        self.rotate_state[n] = is_rotate
        self.blocks.append(np.asarray(block))
        if self._pool is not None:
            return self._pool.request(self._i, np.asarray(block, dtype=np.float32).reshape(-1))
        blk = torch.as_tensor(np.asarray(block, dtype=np.float32).reshape(1, -1))
        feat = self._b.add_new_blocks(blk)
        self._b.check()
        return self._shape(feat)

    def add_new_block_at(self, block, pos_x, is_rotate=False):
        """tools.Container.add_new_block_at (tools.py:3746-3822), what DRL_L's decoding loop calls (model.py:1211): the
        2D block at column ``pos_x`` (clamped to W - w), stability and empty_size by the reference's rules (tapenv.h:
        TAP_AT_CONTAINER).  Returns the heightmap_type feature like add_new_block.  The first call switches a fresh
        Container to the place-at step; mixing it with add_new_block raises NotImplementedError.  Pooled
        (lockstep_scope): one launch per round for the whole pool, ``pos_x`` may be a 0-d device tensor (no host read)."""
        if self._mode == 'block':
            raise NotImplementedError("add_new_block_at on a Container stepped with add_new_block: this package runs "
                                      "one of the two placements per Container, not both")
        if self.block_dim != 2:
            raise NotImplementedError("add_new_block_at is 2D only (tools.py:3762 unpacks two block sides)")
        n = len(self.blocks)
        if n >= self.blocks_num:
            raise IndexError("list assignment index out of range")   # tools.py:3758
        if self._mode is None:
            if self._pool is not None:
                self._pool.use_place_at()
            else:
                (cs, bn, rt, ht, ics, mh, ps, dev) = self._args
                self._b = BatchedContainer(1, cs, bn, rt, ht, ics, mh, ps, dev, place_at='container')
            self._mode = 'at'
        self.rotate_state[n] = is_rotate
        self.blocks.append(np.asarray(block))
        blk = np.asarray(block, dtype=np.float32).reshape(-1)
        if self._pool is not None:
            return self._pool.request(self._i, blk, pos_x)
        feat = self._b.add_new_blocks_at(torch.as_tensor(blk.reshape(1, -1)), torch.as_tensor(pos_x).reshape(1))
        self._b.check()
        return self._shape(feat)

    def get_heightmap(self, is_full=None):
        if is_full is not None:
            return self.heightmap
        if self._pool is not None:
            return self._pool.request(self._i, None)
        return self._shape(self._b.get_heightmaps())

    def calc_CPS(self):
        c, p, s = self._env.calc_CPS()[self._i].tolist()
        return c, p, s

    def calc_ratio(self):
        if self._pool is not None:
            return self._pool.ratio(self._i)
        return float(self._b.calc_ratios64()[0].item())

    def draw_container(self, save_name=None, **kwargs):
        """tools.Container.draw_container (tools.py:3746-3822; called by rolling.py:655 for the first six instances): the
        reference renders the packing with matplotlib.  Drawing is outside this package: the call is
        accepted so that rolling.validate's loop runs unchanged, writes nothing and says so once; everything a drawing
        needs is here -- ``positions``, ``blocks``, ``stable``, ``container`` (the voxel grid, rebuilt on demand)."""
        global _draw_warned
        if not _draw_warned:
            import warnings
            warnings.warn("tap_net_amd.tools.Container.draw_container writes no image (drawing is out of scope); "
                          "positions / blocks / stable / container hold what a renderer needs", stacklevel=2)
            _draw_warned = True

    def clear_container(self):
        if self._pool is not None and self._pool.members > 1:
            raise NotImplementedError("clear_container on one member of a lock-step pool: build new Containers per "
                                      "episode (as model.py:294 does), or switch pooling off for this use")
        self._env.reset()
        if self._pool is not None:
            self._pool.hm_cache = None
        self.blocks = []
        self.rotate_state = [False] * self.blocks_num
        self.bounding_box = np.zeros(self.block_dim)

    @property
    def heightmap(self):
        if self._pool is not None and self._pool.place_at is not None:
            return self._pool.heightmap(self._i)
        return self._env.heightmap[self._i].cpu().numpy().astype(np.int64)

    @property
    def positions(self):
        return self._env.positions[self._i].cpu().numpy().astype(np.int64)

    @property
    def stable(self):
        return [bool(v) for v in self._env.stable[self._i].tolist()]

    @property
    def valid_size(self):
        return int(self._env.counters[self._i, 0].item())

    @property
    def empty_size(self):
        return int(self._env.counters[self._i, 1].item())

    @property
    def current_blocks_num(self):
        return int(self._env.counters[self._i, 3].item())

    @property
    def container(self):
        """Voxel grid rebuilt from the placement history (block ids, -1 for covered holes), the
        array tools.py keeps at self.container; the kernels themselves never materialise it."""
        grid = np.zeros(self.container_size, dtype=np.int64)
        pos, st_blocks = self.positions, [np.asarray(b).astype(int) for b in self.blocks]
        hm = np.zeros(self.container_size[:-1], dtype=np.int64)
        placed_any = np.zeros(len(st_blocks), dtype=bool)
        # a failed placement leaves position 0 and does not touch the height-map; replay to tell
        for i, b in enumerate(st_blocks):
            p = pos[i]
            sl = tuple(slice(int(p[k]), int(p[k]) + int(b[k])) for k in range(self.block_dim - 1))
            if any(int(p[k]) + int(b[k]) > self.container_size[k] for k in range(self.block_dim - 1)):
                continue
            z = int(p[-1])
            if hm[sl].size == 0 or int(hm[sl].max()) != z:
                continue
            placed_any[i] = True
            under = grid[sl + (slice(0, z),)]
            under[under == 0] = -1
            grid[sl + (slice(z, z + int(b[-1])),)] = i + 1
            hm[sl] = z + int(b[-1])
        return grid
