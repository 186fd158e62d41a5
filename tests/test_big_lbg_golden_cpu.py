"""The oracle against the reference's own LB_GREEDY episodes on a container above 4 096 cells (70 x 70,
tests/golden/big_lbg.npz from make_golden_big.py): pins the oracle the big-container GPU tests compare with at the new
sizes.  (The 2D traces of the fixture, 5 000 and 16 384 columns, are beyond the oracle's 4 096 columns; the GPU tests
compare the library with them directly.)"""
import os

import numpy as np

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "big_lbg.npz")


def test_oracle_matches_reference_above_4096_cells():
    z = np.load(GOLDEN)
    cases = [str(c) for c in z["cases"] if str(c).startswith("c")]
    assert cases
    for case in cases:
        cs = [int(v) for v in z[case + "_cs"]]
        reward = str(z[case + "_reward"])
        for e, blocks in enumerate(z[case + "_blocks"]):
            rc, pos, st, ratio, scores = O.calc_positions_lb_greedy(blocks, cs, reward)
            assert rc == 0, (case, e)
            assert np.array_equal(pos, z[case + "_positions"][e]), (case, e)
            assert np.array_equal(np.asarray(st, np.uint8), z[case + "_stable"][e]), (case, e)
            assert ratio == z[case + "_ratio"][e], (case, e)
            assert np.array_equal(np.asarray(scores, np.int64), z[case + "_scores"][e]), (case, e)
