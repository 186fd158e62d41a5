"""Numpy restatement of the global pack-net's engine (tapenv.h: tap_env_step_engine), batched over instances.

It restates pack_net/LG_RL.py's PackEngine (LG_RL.py:414-528) with add_block (LG_RL.py:126-192): blocks truncated, the
column clamped to W - w, z = max(heightmap[x:x+w]), stability of the support row, empty_size = sum(heightmap) -
valid_size, the per-step reward (C+P+S)/3 in float64 cast to float32, and the wrap: after the step that makes
time == max_blocks_num the engine clears, the reward and the tape keep the values from before.  Pinned to the
reference's traces by tests/golden/pack_rnn.npz (make_golden_pack_rnn.py).

With ``grid=True`` every instance also keeps the reference's container array and steps it with LG_RL's add_block and
is_stable_2d as written; each step then asserts that the height-map rules above give the same stability and the same
empty_size ((container != 0).sum() - valid_size).  That mode is for small batches (the fixture's).

Divergences of the package, restated here too: a block narrower than 1 cell, wider than the container or at a column
< 0 sets error bit 4 and is not placed (its tape entry is (0, 0), unstable; the step still counts in S's denominator,
as PackEngine counts every step with a non-zero width); z + h > H sets error bit 1 (the reference clips its numpy
slices) and is placed.  The error word restarts at step 0.
"""
import numpy as np
import torch


def is_stable_2d(support, obj_left, obj_width):
    """LG_RL.is_stable_2d (LG_RL.py:94-124), literally: cells <= 0 are empty, a width-1 block on a filled cell is
    stable"""
    object_center = obj_left + obj_width / 2
    left_index = obj_left
    right_index = obj_left + obj_width
    for left in support:
        if left <= 0:
            left_index += 1
        else:
            break
    for right in reversed(support):
        if right <= 0:
            right_index -= 1
        else:
            break
    if left_index + 1 == right_index and obj_width == 1:
        return True
    if object_center <= left_index or object_center >= right_index:
        return False
    return True


def heightap(hm, heightmap_type):
    """PackEngine.get_heightap (LG_RL.py:498-515) of (B, W) height-maps -> (B, W') int64: W, or W - 1 for 'diff'"""
    hm = np.asarray(hm, np.int64)
    if heightmap_type == 'full':
        return hm.copy()
    if heightmap_type == 'zero':
        return hm - hm.min(axis=1, keepdims=True)
    if heightmap_type == 'diff':
        return hm[:, 1:] - hm[:, :-1]
    raise ValueError(heightmap_type)


def reward(valid, empty, nstable, count, hmax, W):
    """PackEngine.step's reward (LG_RL.py:460-475) per instance, float64: each term 0 when its denominator is 0
    (elementwise IEEE division, the same roundings as the reference's scalar numpy divisions)"""
    valid, ve = np.asarray(valid, np.int64), np.asarray(valid, np.int64) + np.asarray(empty, np.int64)
    box, count = np.asarray(hmax, np.int64) * W, np.asarray(count, np.int64)

    def ratio(num, den):
        return np.where(den == 0, 0.0, np.asarray(num, np.int64) / np.where(den == 0, 1, den))
    return (ratio(valid, box) + ratio(valid, ve) + ratio(nstable, count)) / 3


class PackEngines(object):
    """B engines W x H, tape of T steps, wrap every max_blocks_num steps (0 = never).  The surface of
    tap_net_amd.env.PackEngines, so a tools.PackRNN can run on it (engine=PackEngines): step() returns torch tensors on
    ``device``."""

    def __init__(self, batch_size, container_width, container_height, T, heightmap_type='diff', max_blocks_num=10,
                 device='cpu', grid=False):
        self.batch_size, self.W, self.H, self.T = int(batch_size), int(container_width), int(container_height), int(T)
        self.heightmap_type, self.max_blocks_num = heightmap_type, int(max_blocks_num)
        self.device = torch.device(device)
        self.grid = grid
        B, W = self.batch_size, self.W
        self.hm = np.zeros((B, W), np.int64)
        self.valid = np.zeros(B, np.int64)
        self.nstable = np.zeros(B, np.int64)
        self.count = np.zeros(B, np.int64)
        self.err = np.zeros(B, np.int64)
        self.pos = np.zeros((B, self.T, 2), np.int64)
        self.stab = np.zeros((B, self.T), np.uint8)
        self.rw64 = np.zeros(B, np.float64)
        self.reward = torch.zeros(B, dtype=torch.float32, device=self.device)
        self.launches = 0
        self.tape_len = 0
        self.last_input = None
        self._clear_grid()

    def _clear_grid(self):
        if self.grid:
            self.container = np.zeros((self.batch_size, self.W, self.H))

    def reset(self):
        self.hm[:] = 0
        self.valid[:] = 0
        self.nstable[:] = 0
        self.count[:] = 0
        self._clear_grid()
        self.last_input = None

    @property
    def empty(self):
        return self.hm.sum(axis=1) - self.valid

    def counters(self):
        """the blob's counters: valid, empty, stable blocks since the clear, and the forward's tape length"""
        return np.stack((self.valid, self.empty, self.nstable, np.full(self.batch_size, self.tape_len, np.int64)), 1)

    def step(self, i, blocks, x, want_reward=True, out=None, want_input=True):
        B, W, M = self.batch_size, self.W, self.max_blocks_num
        i = int(i)
        bl = blocks.detach().cpu().numpy() if isinstance(blocks, torch.Tensor) else np.asarray(blocks)
        bl = np.trunc(np.asarray(bl, np.float64)[:, :, i]).astype(np.int64)          # block.int(), LG_RL.py:450
        xs = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.int64).reshape(B)
        self.launches += 1
        if (i % M == 0) if M else i == 0:                                             # the clear / the wrap
            self.reset()
        if i == 0:
            self.err[:] = 0
        w, h = bl[:, 0], bl[:, 1]
        ok = (w >= 1) & (h >= 1)
        xl = np.minimum(xs, W - w)                                                    # while x + w > W: x -= 1
        ok &= xl >= 0
        self.err[~ok] |= 4
        x0 = np.where(ok, xl, 0)
        ww = np.where(ok, w, 0)
        c = np.arange(W)[None, :]
        inb = (c >= x0[:, None]) & (c < (x0 + ww)[:, None])
        z = np.where(inb, self.hm, 0).max(axis=1)
        eq = inb & (self.hm == z[:, None])                                            # support cells that carry it
        first = np.argmax(eq, axis=1)
        last = W - 1 - np.argmax(eq[:, ::-1], axis=1)
        lead, trail = first - x0, (x0 + ww - 1) - last
        stab = ((z == 0) | ((2 * lead < ww) & (2 * trail < ww))).astype(np.int64)
        if self.grid:
            self._grid_step(ok, x0, z, w, h, stab)
        self.hm = np.where(inb & ok[:, None], (z + h)[:, None], self.hm)
        self.err[ok & (z + h > self.H)] |= 1
        idx = np.nonzero(ok)[0]
        self.pos[:, i] = 0                                                            # (0, 0), unstable, if refused
        self.stab[:, i] = 0
        self.pos[idx, i, 0] = x0[idx]
        self.pos[idx, i, 1] = z[idx]
        self.stab[idx, i] = stab[idx]
        self.valid[idx] += w[idx] * h[idx]
        self.nstable[idx] += stab[idx]
        self.count += 1                                   # PackEngine.num_blocks: every step since the clear counts
        self.tape_len = i + 1
        if self.grid:
            py = (self.container != 0).sum(axis=(1, 2)) - (self.container >= 1).sum(axis=(1, 2))
            assert np.array_equal(py, self.empty), (py, self.empty)
        if want_reward:
            self.rw64 = reward(self.valid, self.empty, self.nstable, self.count, self.hm.max(axis=1), W)
            self.reward = torch.as_tensor(self.rw64.astype(np.float32), device=self.device)
        self.pre_hm, self.pre_valid, self.pre_empty = self.hm.copy(), self.valid.copy(), self.empty
        if M and (i + 1) % M == 0:                                                    # time == max_blocks_num
            self.reset()
        if not want_input:
            self.last_input = None
            return None
        self.last_input = self.get_heightaps(self.heightmap_type)
        return self.last_input

    def _grid_step(self, ok, x0, z, w, h, stab):
        """LG_RL.add_block (LG_RL.py:158-177) on every instance's container, literally"""
        for b in np.nonzero(ok)[0]:
            cont, x, zz, bw, bh = self.container[b], int(x0[b]), int(z[b]), int(w[b]), int(h[b])
            if zz == 0:
                st = True
            else:
                st = is_stable_2d(cont[x:x + bw, zz - 1], x, bw)
            assert int(st) == int(stab[b]), (b, x, zz, bw)
            cont[x:x + bw, zz:zz + bh] = self.count[b] + 1
            under = cont[x:x + bw, :zz]
            cont[x:x + bw, :zz][under == 0] = -1

    def get_heightaps(self, heightmap_type):
        return torch.as_tensor(heightap(self.hm, heightmap_type).astype(np.float32), device=self.device).unsqueeze(2)

    @property
    def positions(self):
        return torch.as_tensor(self.pos.astype(np.int32), device=self.device)

    @property
    def stable(self):
        return torch.as_tensor(self.stab.astype(bool), device=self.device)

    @property
    def errors(self):
        return torch.as_tensor(self.err.astype(np.int32), device=self.device)

    def check(self):
        if self.err.any():
            raise IndexError("engine error bits %s" % (np.unique(self.err[self.err != 0]).tolist(),))


def factory(grid=False, device=None):
    """an engine factory for tools.PackRNN(..., engine=...): the numpy restatement on ``device`` (default: where the
    blocks are)"""
    def make(B, W, H, T, heightmap_type, max_blocks_num, dev):
        return PackEngines(B, W, H, T, heightmap_type, max_blocks_num, device if device is not None else dev, grid=grid)
    return make
