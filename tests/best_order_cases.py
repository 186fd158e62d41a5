"""Shared by tests/test_best_order_cpu.py and tests/test_trial_scores_gpu.py: the best-order fixture
(tests/golden/best_order.npz, written by tests/golden/make_golden_best_order.py from the reference's
generate_order_graph(..., 'best')) and the oracle restatement of one trial and of the greedy loop -- a fresh oracle
Env replaying the committed blocks plus the candidate, scored with fp64 calc_ratio, the first strict maximum taken."""
import os

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "best_order.npz"))
K = len(Z["n"])


class Case(object):
    def __init__(self, k):
        n, D = int(Z["n"][k]), int(Z["D"][k])
        self.k, self.n, self.D = k, n, D
        self.blocks = Z["blocks"][k, :n, :D].astype(np.int32)
        self.positions = Z["positions"][k, :n, :D].astype(np.int32)
        self.initial = [int(v) for v in Z["initial"][k, :D]]
        self.target = [int(v) for v in Z["target"][k, :D]]
        self.reward_type = str(Z["reward_type"][k])
        self.allow_bot = bool(Z["allow_bot"][k])
        self.solution = [int(v) for v in Z["solution"][k, :n]]
        self.mean_valid = float(Z["mean_valid"][k])

    @property
    def id(self):
        return "%02d-%dd-%s-n%d-%s%s" % (self.k, self.D, "x".join(str(v) for v in self.initial[:-1]), self.n,
                                         self.reward_type.split("-", 1)[1], "" if self.allow_bot else "-nobot")

    @property
    def lane_kernel(self):
        """does the one-launch trial kernel take this case (LB_GREEDY)?"""
        return "-lb-" in self.reward_type


CASES = [Case(k) for k in range(K)]


def trial_score(target, n_max, reward_type, committed, block):
    """fp64 calc_ratio of a fresh container after ``committed`` + ``block``; -1.0 when the candidate's step raises"""
    e = O.Env(target, n_max, reward_type, "full")
    for b in committed:
        rc, _ = e.add_new_block(b)
        assert rc == 0 and e.error == 0, "a committed block raised"
    rc, _ = e.add_new_block(block)
    return -1.0 if (rc != 0 or e.error != 0) else e.calc_ratio()


def trial_row(target, n_max, reward_type, committed, static, cur_mask):
    """(scores (nR,) float64, best) for one env: -inf for the unselectable columns, numpy's first maximum"""
    nR = static.shape[1]
    scores = np.full(nR, -np.inf)
    for c in np.flatnonzero(cur_mask):
        scores[c] = trial_score(target, n_max, reward_type, committed, static[1:, c].astype(np.int32))
    return scores, int(np.argmax(scores))


def instance(case):
    """(static (1+D, nR), dynamic (rows, nR), update_rows) of a fixture case from the oracle's own packing"""
    rc, pos, st, dyn = O.instance_from_blocks(case.blocks, case.initial, 1)
    assert rc == 1 and np.array_equal(pos, case.positions)
    if not case.allow_bot:
        return st, np.ascontiguousarray(dyn[:case.n]), 1        # input type 'rot': the movement rows only
    return st, dyn, 3


def greedy(case):
    """the greedy best-ratio loop on the oracle alone -> (solution, mean_valid, per-step (cur_mask, scores))"""
    st, dyn, upd = instance(case)
    n, R = case.n, st.shape[1] // case.n
    dyn = dyn[None].copy()
    cur = O.initial_mask(dyn, n)
    mask = np.ones_like(cur)
    committed, solution, valid, steps = [], [], [], []
    for _ in range(n):
        scores, best = trial_row(case.target, n, case.reward_type, committed, st, cur[0])
        # the reference's rule (generate.py:1262-1279): the first node whose ratio is strictly larger than all before
        top, pick = 0.0, int(np.flatnonzero(cur[0])[0])
        for c in np.flatnonzero(cur[0]):
            if top < scores[c]:
                top, pick = scores[c], int(c)
        assert pick == best or scores[best] <= 0.0
        valid.append(int(cur[0].sum()))
        steps.append((cur[0].copy(), scores))
        solution.append(pick)
        committed.append(st[1:, pick].astype(np.int32))
        ptr = np.asarray([pick], np.int64)
        dyn = O.update_dynamic(dyn, st[None], ptr, n, upd)
        cur, mask = O.update_mask(mask, dyn, ptr, n, R)
    return solution, float(np.mean(valid)), steps
