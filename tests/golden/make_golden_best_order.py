#!/usr/bin/env python3
"""Generate tests/golden/best_order.npz by running the UPSTREAM REFERENCE's greedy best-ratio order:
generate.generate_order_graph(blocks, positions, initial_size, 1, allow_bot, 'best', reward_type, target_size)
(generate.py:1109-1361) on instances drawn by its own generate.generate_blocks under recorded seeds.

Per case: blocks (rotation 0) and positions (n, D), the initial and the target container size, the reward type,
allow_bot, the seed, and the reference's `solution` (node ids rot * n + block) and `mean_valid_nodes_num`.  Arrays are
padded to the largest n / D (blocks and positions with 0, solution with -1).  Like make_golden.py it runs only where
the reference checkout is present.  Usage:

    python tests/golden/make_golden_best_order.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402

SOFT, HARD = 'C+P+S-lb-soft', 'C+P+S-lb-hard'
SHAPES = [([5, 50], [5, 50]), ([7, 50], [5, 50]), ([5, 5, 50], [5, 5, 50])]     # (initial, target)


def cases():
    """(initial, target, n, reward_type, allow_bot, seed)"""
    out = []
    seed = 4100
    for init, target in SHAPES:
        for n in (6, 10):
            for rt in (SOFT, HARD):
                for _ in range(4):
                    out.append((init, target, n, rt, True, seed))
                    seed += 1
    for init, target, n, rt in (([5, 50], [5, 50], 10, 'C+P+S-mcs-soft'), ([7, 50], [5, 50], 6, 'C+P+S-mcs-soft'),
                                ([5, 50], [5, 50], 10, 'C+P+S-mul-soft'), ([7, 50], [5, 50], 6, 'C+P+S-mul-soft'),
                                ([5, 5, 50], [5, 5, 50], 6, 'C+P+S-mcs-soft')):
        out.append((init, target, n, rt, True, seed))
        seed += 1
    for init, target, n, rt in (([5, 50], [5, 50], 10, SOFT), ([5, 50], [5, 50], 10, SOFT), ([7, 50], [5, 50], 6, HARD),
                                ([5, 5, 50], [5, 5, 50], 6, SOFT), ([5, 5, 50], [5, 5, 50], 6, SOFT),
                                ([5, 5, 50], [5, 5, 50], 10, HARD)):
        out.append((init, target, n, rt, False, seed))
        seed += 1
    return out


def main():
    mods = ref_loader.load()
    if mods is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    generate = mods[2]
    cs = cases()
    K, N = len(cs), max(c[2] for c in cs)
    blocks = np.zeros((K, N, 3), np.int32)
    positions = np.zeros((K, N, 3), np.int32)
    init = np.zeros((K, 3), np.int32)
    target = np.zeros((K, 3), np.int32)
    solution = np.full((K, N), -1, np.int64)
    mean_valid = np.zeros(K, np.float64)
    for k, (ini, tgt, n, rt, allow_bot, seed) in enumerate(cs):
        D = len(ini)
        np.random.seed(seed)
        rot_blocks, pos, _, _, _ = generate.generate_blocks(n, list(ini), 1, [1, 5])
        b = np.asarray(rot_blocks)[0].reshape(D, n).T.astype(np.int32)             # rotation 0 (generate.py:951)
        p = np.asarray(pos).reshape(D, n).T.astype(np.int32)                       # generate.py:967-968
        sol, _, mv = generate.generate_order_graph(b.copy(), p.copy(), list(ini), 1, allow_bot, 'best', rt, list(tgt))
        assert len(sol) == n and sorted(int(s) % n for s in sol) == list(range(n))
        blocks[k, :n, :D], positions[k, :n, :D] = b, p
        init[k, :D], target[k, :D] = ini, tgt
        solution[k, :n] = [int(s) for s in sol]
        mean_valid[k] = float(mv)
    np.savez_compressed(os.path.join(HERE, "best_order.npz"), blocks=blocks, positions=positions,
                        n=np.asarray([c[2] for c in cs], np.int32), D=np.asarray([len(c[0]) for c in cs], np.int32),
                        initial=init, target=target, reward_type=np.asarray([c[3] for c in cs]),
                        allow_bot=np.asarray([c[4] for c in cs], np.uint8), seed=np.asarray([c[5] for c in cs], np.int64),
                        solution=solution, mean_valid=mean_valid)
    print("%d cases" % K)


if __name__ == "__main__":
    main()
