"""The model of the fused pointer launch (tapenv.h: tap_pointer_pick_static) in numpy: pointer_static_model's static term and
pointer_model's folded contract give the logits, policy_head_model / policy_head_forms_model pick from them.  What
tests/test_rolling_actor_cpu.py and tests/test_pointer_pick_static_gpu.py share.

    fused               -> ptr (B,) int64, logp (B,) fp64, logits (B, nR): greedy, or DRAW at (seed, episode, step, env_offset)
    make_case           a case of the GPU comparison: pointer_static_model.make_case plus a random current_mask in which a few
                        rows are forced empty and every other row has a selectable column
    SHAPES              the (B, nR, rows, Hd, S) of the GPU comparison and what each exercises"""
import numpy as np

import policy_head_forms_model as FM
import policy_head_model as HM
import pointer_model as PM
import pointer_static_model as SM

SHAPES = [
    (19, 20, 30, 64, 2),        # c5's window
    (19, 20, 30, 128, 2),       # two hidden rows per lane
    (19, 60, 30, 256, 3),       # the 3D window, two chunks
    (19, 68, 63, 64, 2),        # the head's second 64-column chunk
    (19, 4, 65, 128, 4),        # two shadow planes, synthetic shadow only
    (19, 20, 30, 128, 5),       # the LDS copy of G
    (3074, 20, 30, 128, 2),     # three envs per workgroup, ragged last one
    (5123, 4, 10, 64, 2),       # five envs, more than the four wavefronts
]
EMPTY_ROWS = (2, 7, 11)         # rows of the mask forced empty (those the batch has)


def fused(xs, G, g, dyn, M, k, q, va, vp, mask, draw=None, dtype=np.float64):
    """``dyn`` (B, rows, nR) 0/1; ``draw`` None (greedy) or (seed, episode, step[, env_offset]).  Every operation of the scores
    in ``dtype``; the head in fp64 on those logits, as the kernels' head is"""
    P = SM.static_term(xs, G, g, dtype)
    logits = PM.folded(P, dyn, M, k, q, va, vp, dtype)[0]
    if draw is None:
        ptr, logp = HM.pick(logits, mask, None)[:2]
    else:
        ptr, logp = FM.draw(logits, mask, *draw)[:2]
    return ptr, logp, logits


def random_mask(B, nR, seed):
    """(B, nR) float32 of 0 / 1 at 40 %: EMPTY_ROWS empty, every other row with at least one selectable column"""
    rng = np.random.RandomState(seed)
    mask = (rng.rand(B, nR) < 0.4).astype(np.float32)
    mask[np.arange(B), rng.randint(0, nR, size=B)] = 1
    for b in EMPTY_ROWS:
        if b < B:
            mask[b] = 0
    return mask


def make_case(B, nR, rows, Hd, S, seed=0, He=None):
    """-> dict: pointer_static_model.make_case's entries, the float32 fold (G, g, M, k, q), the shadow ``bits`` and ``mask``"""
    X = SM.make_case(B, rows, nR, Hd // 2 if He is None else He, Hd, S, 0.3, 4000 + seed)
    G, g, M, k, q = (np.asarray(a, np.float32) for a in SM.fold(X, np.float64))
    X.update(G=G, g=g, M=M, k=k, q=q, bits=PM.pack_bits(X["dyn"]), mask=random_mask(B, nR, 9000 + seed))
    return X
