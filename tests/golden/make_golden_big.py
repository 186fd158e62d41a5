#!/usr/bin/env python3
"""Generate tests/golden/big_lbg.npz by running the UPSTREAM REFERENCE's tools.calc_positions_lb_greedy on containers
above 4 096 cells: 2D containers of 5 000 and 16 384 columns and a 3D one of 70 x 70, soft and hard rewards, a few short episodes
each.  Like make_golden.py it runs only where the reference checkout is present; the fixture holds the inputs and the
reference's outputs only.  Usage:

    python tests/golden/make_golden_big.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402

# (name, container_size, reward_type, episodes, n, block side range, height range)
CASES = [
    ("w5000_soft", [5000, 40], "C+P+S-lb-soft", 6, 6, (200, 1600), (1, 8)),
    ("w5000_hard", [5000, 40], "C+P+S-lb-hard", 6, 6, (200, 1600), (1, 8)),
    ("w16384_hard", [16384, 30], "C+P+S-lb-hard", 4, 6, (500, 6000), (1, 8)),
    ("c70_soft", [70, 70, 40], "C+P+S-lb-soft", 6, 6, (5, 17), (1, 8)),
    ("c70_hard", [70, 70, 40], "C+P+S-lb-hard", 6, 6, (5, 17), (1, 8)),
]


def main():
    mods = ref_loader.load()
    if mods is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    tools = mods[0]
    out = {}
    for name, cs, reward, E, n, (lo, hi), (hlo, hhi) in CASES:
        rs = np.random.RandomState(sum(map(ord, name)))
        D = len(cs)
        blocks = rs.randint(lo, hi, size=(E, n, D)).astype(np.int32)
        blocks[:, :, -1] = rs.randint(hlo, hhi, size=(E, n))
        pos = np.zeros((E, n, D), np.int32)
        st = np.zeros((E, n), np.uint8)
        ratio = np.zeros(E, np.float64)
        scores = np.zeros((E, 5), np.int64)
        for e in range(E):
            p, _, s, r, sc = tools.calc_positions_lb_greedy(blocks[e].copy(), list(cs), reward)
            pos[e], st[e], ratio[e], scores[e] = np.asarray(p), np.asarray(s, np.uint8), float(r), np.asarray(sc, np.int64)
        out[name + "_cs"] = np.asarray(cs, np.int32)
        out[name + "_reward"] = np.asarray(reward)
        out[name + "_blocks"] = blocks
        out[name + "_positions"] = pos
        out[name + "_stable"] = st
        out[name + "_ratio"] = ratio
        out[name + "_scores"] = scores
        print(name, "done", flush=True)
    out["cases"] = np.asarray([c[0] for c in CASES])
    np.savez_compressed(os.path.join(HERE, "big_lbg.npz"), **out)


if __name__ == "__main__":
    main()
