"""Numpy restatement of the pack-net placement (tapenv.h: tap_env_step_at), batched over containers.

The two seams of the reference it restates, pinned to them by tests/golden/place_at.npz:
  'container'  tools.Container.add_new_block_at (tools.py:3746-3822): every block is stable (the support row is read
               after the cells under the block were filled), empty_size += sum over the block's columns of
               (z - block cells of the column)
  'net'        tools.calc_one_position_net (tools.py:3371-3461): tools.is_stable_2d on the support row before the
               fill, empty_size = sum(heightmap) - valid_size
Divergences of the package, restated here too: a block wider than the container or a column < 0 sets error bit 4 and
is not placed; z + h > H sets error bit 1 (the reference clips silently) and is placed.
"""
import numpy as np


def is_stable_2d(support, obj_left, obj_width):
    """tools.is_stable_2d (tools.py:839-868) on a support row (0 = empty)"""
    center = obj_left + obj_width / 2
    left, right = obj_left, obj_left + obj_width
    for v in support:
        if v == 0:
            left += 1
        else:
            break
    for v in reversed(support):
        if v == 0:
            right -= 1
        else:
            break
    return not (center <= left or center >= right)


def feature(hm, heightmap_type):
    """Container's decoder feature (tools.py:3802-3821) of (B, W) height-maps -> (B, flen): W, or W - 1 for 'diff'"""
    hm = np.asarray(hm, np.int64)
    if heightmap_type == 'full':
        return hm.copy()
    if heightmap_type == 'zero':
        return hm - hm.min(axis=1, keepdims=True)
    return hm[:, 1:] - hm[:, :-1]


def pnet_input(hm, form):
    """the pack-net's input (B, W): 'full' the raw map (tools.py:3407), 'zero' minus its minimum, 'diff'
    hm[c+1] - hm[c] with a trailing 0 (DRL_L, model.py:1188-1192)"""
    hm = np.asarray(hm, np.int64)
    if form == 'full':
        return hm.copy()
    if form == 'zero':
        return hm - hm.min(axis=1, keepdims=True)
    out = np.zeros_like(hm)
    out[:, :-1] = hm[:, 1:] - hm[:, :-1]
    return out


class PlaceAt(object):
    """B containers W x H stepped with blocks at given columns"""

    def __init__(self, B, W, H, n_max, semantics):
        assert semantics in ('container', 'net')
        self.B, self.W, self.H, self.n_max, self.sem = B, W, H, n_max, semantics
        self.hm = np.zeros((B, W), np.int64)
        self.col = np.zeros((B, W), np.int64)
        self.valid = np.zeros(B, np.int64)
        self.empty = np.zeros(B, np.int64)
        self.nstable = np.zeros(B, np.int64)
        self.count = np.zeros(B, np.int64)
        self.err = np.zeros(B, np.int64)
        self.positions = np.zeros((B, n_max, 2), np.int64)
        self.stable = np.zeros((B, n_max), np.uint8)

    def counters(self):
        return np.stack((self.valid, self.empty, self.nstable, self.count), 1)

    def step(self, blocks, pos_x, active=None):
        """blocks (B, 2) -- truncated like block.astype(int) --, pos_x (B,) ints, active (B,) or None"""
        B, W = self.B, self.W
        blocks = np.trunc(np.asarray(blocks, np.float64)).astype(np.int64).reshape(B, 2)
        w, h = blocks[:, 0], blocks[:, 1]
        xs = np.asarray(pos_x, np.int64).reshape(B)
        act = np.ones(B, bool) if active is None else np.asarray(active).astype(bool).reshape(B)
        e2 = act & (self.count >= self.n_max)
        self.err[e2] |= 2
        ok = act & ~e2
        e4 = ok & ((w < 1) | (h < 1))
        ok &= ~e4
        xl = np.minimum(xs, W - w)                              # while x + w > W: x -= 1
        e4 |= ok & (xl < 0)
        self.err[e4] |= 4
        ok &= ~e4
        x = np.where(ok, xl, 0)
        ww = np.where(ok, w, 0)
        c = np.arange(W)[None, :]
        inb = (c >= x[:, None]) & (c < (x + ww)[:, None])
        z = np.where(inb, self.hm, 0).max(axis=1)
        if self.sem == 'container':
            stab = np.ones(B, np.int64)
            dempty = np.where(inb, z[:, None] - self.col, 0).sum(axis=1)
            self.col = np.where(inb, self.col + h[:, None], self.col)
        else:
            # is_stable_2d on the support row (column tops equal to z), for all containers at once: the centre must
            # lie strictly between the first and one past the last supporting column
            eq = inb & (self.hm == z[:, None])
            first = np.argmax(eq, axis=1)
            last = W - 1 - np.argmax(eq[:, ::-1], axis=1)
            lead, trail = first - x, (x + ww - 1) - last
            stab = ((z == 0) | ((2 * lead < ww) & (2 * trail < ww))).astype(np.int64)
        self.hm = np.where(inb, (z + h)[:, None], self.hm)
        self.err[ok & (z + h > self.H)] |= 1
        idx = np.nonzero(ok)[0]
        t = self.count[idx]
        self.positions[idx, t, 0] = x[idx]
        self.positions[idx, t, 1] = z[idx]
        self.stable[idx, t] = stab[idx]
        self.valid[idx] += w[idx] * h[idx]
        self.nstable[idx] += stab[idx]
        self.count[idx] += 1
        if self.sem == 'container':
            self.empty[idx] += dempty[idx]
        else:
            self.empty[idx] = self.hm[idx].sum(axis=1) - self.valid[idx]

    def ratio(self):
        """Container.calc_ratio for the SL / RL types: (C + P + S) / 3 (tools.py:3887-3966), float64"""
        out = np.zeros(self.B, np.float64)
        for b in range(self.B):
            if self.count[b] == 0:
                continue
            box = self.W * int(self.hm[b].max())
            C = float(self.valid[b]) / box
            P = float(self.valid[b]) / float(self.empty[b] + self.valid[b])
            S = float(self.nstable[b]) / float(self.count[b])
            out[b] = (C + P + S) / 3
        return out

    def scores(self, n):
        """calc_positions_net's (ratio, [valid, box, empty, stable_num, max_h]) after n blocks (tools.py:3576-3598)"""
        ratio = np.zeros(self.B, np.float64)
        sc = np.zeros((self.B, 5), np.int64)
        for b in range(self.B):
            mh = int(self.hm[b].max())
            box = mh * self.W
            sc[b] = (self.valid[b], box, self.empty[b], self.nstable[b], mh)
            if n:
                C = self.valid[b] / np.float64(box)
                P = self.valid[b] / np.float64(self.empty[b] + self.valid[b])
                S = np.float64(self.nstable[b]) / n
                ratio[b] = (C + P + S) / 3
        return ratio, sc
