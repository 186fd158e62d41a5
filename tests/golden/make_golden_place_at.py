#!/usr/bin/env python3
"""Generate tests/golden/place_at.npz by running the UPSTREAM REFERENCE's pack-net seams:
  - tools.Container.add_new_block_at for W in {1, 2, 5, 7, 10, 16, 31, 64}, every heightmap_type, columns that include
    x >= W (clamped by the reference): per step the returned feature, positions, stable, valid_size, empty_size and
    calc_ratio;
  - tools.calc_positions_net (-> calc_one_position_net) on the same kind of cases, its net replaced by a stub that
    returns the recorded column (one-hot) and records the height-map and block it was shown;
  - tools.DQN's outputs for seeded random weights (both input forms, W = 5, eval mode), with the parameter names and
    shapes (the weights are rebuilt from the seed by the test).
Like make_golden.py it runs only where the reference checkout is present; while it runs, Tensor.cuda / Module.cuda
are the identity (the reference moves every tensor to the GPU) -- that patch stays here.  Usage:

    python tests/golden/make_golden_place_at.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402

WIDTHS = (1, 2, 5, 7, 10, 16, 31, 64)
TYPES = ('full', 'zero', 'diff')
N = 12


def draw(rs, W, n):
    blocks = np.stack((rs.randint(1, W + 1, size=n), rs.randint(1, 5, size=n)), 1).astype(np.int32)
    xs = rs.randint(0, W + 4, size=n).astype(np.int64)          # x >= W - w + 1 is clamped by the reference
    return blocks, xs


def main():
    mods = ref_loader.load()
    if mods is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    tools = mods[0]
    import torch
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    out = {}
    names = []
    # ---- Container.add_new_block_at ----------------------------------------------------------------------------
    for W in WIDTHS:
        for t in TYPES:
            name = "c_w%d_%s" % (W, t)
            rs = np.random.RandomState(sum(map(ord, name)))
            blocks, xs = draw(rs, W, N)
            H = 4 * N + 1
            c = tools.Container([W, H], N, 'C+P+S-SL-soft', t)
            feats, hms, vs, es, rs_ = [], [], [], [], []
            for i in range(N):
                f = c.add_new_block_at(blocks[i].astype(np.float32), int(xs[i]))
                feats.append(np.array(f, np.int64).reshape(-1))    # copy: the full form is self.heightmap itself
                hms.append(np.asarray(c.heightmap, np.int64).copy())
                vs.append(int(c.valid_size))
                es.append(int(c.empty_size))
                rs_.append(float(c.calc_ratio()))
            out[name + "_cs"] = np.asarray([W, H], np.int32)
            out[name + "_blocks"] = blocks
            out[name + "_x"] = xs
            out[name + "_feature"] = np.stack(feats) if feats[0].size else np.zeros((N, 0), np.int64)
            out[name + "_hm"] = np.stack(hms)
            out[name + "_positions"] = np.asarray(c.positions, np.int64)
            out[name + "_stable"] = np.asarray(c.stable, np.uint8)
            out[name + "_valid"] = np.asarray(vs, np.int64)
            out[name + "_empty"] = np.asarray(es, np.int64)
            out[name + "_ratio"] = np.asarray(rs_, np.float64)
            names.append(name)
    # ---- calc_positions_net with a scripted net ----------------------------------------------------------------
    real_dqn, real_load = tools.DQN, torch.load
    for W in WIDTHS:
        name = "n_w%d" % W
        rs = np.random.RandomState(sum(map(ord, name)))
        blocks, xs = draw(rs, W, N)
        H = 4 * N + 1
        seen_hm, seen_blk = [], []

        class Scripted(object):
            def __init__(self, *a, **k):
                self.i = 0

            def cuda(self):
                return self

            def eval(self):
                return self

            def load_state_dict(self, *a, **k):
                return None

            def __call__(self, hm, blk):
                seen_hm.append(hm.numpy().reshape(-1).copy())
                seen_blk.append(blk.numpy().reshape(-1).copy())
                p = torch.zeros(1, W + 4)
                p[0, int(xs[self.i])] = 1.0
                self.i += 1
                return p

        tools.DQN = Scripted
        torch.load = lambda *a, **k: {}
        try:
            pos, _, st, ratio, scores = tools.calc_positions_net(blocks.copy(), [W, H], 'C+P+S-SL-soft')
        finally:
            tools.DQN, torch.load = real_dqn, real_load
        out[name + "_cs"] = np.asarray([W, H], np.int32)
        out[name + "_blocks"] = blocks
        out[name + "_x"] = xs
        out[name + "_pnet"] = np.stack(seen_hm).astype(np.float32)      # the raw map the net saw before each block
        out[name + "_netblock"] = np.stack(seen_blk).astype(np.float32)
        out[name + "_positions"] = np.asarray(pos, np.int64)
        out[name + "_stable"] = np.asarray(st, np.uint8)
        out[name + "_ratio"] = np.float64(ratio)
        out[name + "_scores"] = np.asarray([int(v) for v in scores], np.int64)
        names.append(name)
    # ---- DQN ---------------------------------------------------------------------------------------------------
    for diff in (True, False):
        torch.manual_seed(7 if diff else 8)
        net = tools.DQN(5, diff)
        for bn in (net.bn1, net.bn2, net.bn3):       # non-trivial running statistics for the eval-mode forward
            bn.running_mean.uniform_(-0.5, 0.5)
            bn.running_var.uniform_(0.5, 2.0)
        net.eval()
        hm = torch.randint(-3, 8, (6, 1, 5)).float()
        blk = torch.randint(1, 5, (6, 1, 2)).float()
        with torch.no_grad():
            y = net(hm, blk)
        key = "dqn_%s" % ("diff" if diff else "full")
        # the weights themselves are too large for a fixture: the test rebuilds them from the same seed (same layers,
        # same construction order) and checks the names and shapes against these
        sd = net.state_dict()
        out[key + "_sd_keys"] = np.asarray(list(sd))
        out[key + "_sd_shapes"] = np.asarray([",".join(str(d) for d in v.shape) for v in sd.values()])
        out[key + "_hm"] = hm.numpy()
        out[key + "_block"] = blk.numpy()
        out[key + "_out"] = y.numpy()
    out["cases"] = np.asarray(names)
    np.savez_compressed(os.path.join(HERE, "place_at.npz"), **out)


if __name__ == "__main__":
    main()
