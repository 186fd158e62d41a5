"""The DRAW and GIVEN forms of the decoding head (tapenv.h: tap_policy_pick_draw / tap_policy_pick_given) restated in numpy:
the oracle of tests/test_policy_head_forms_cpu.py and tests/test_policy_head_forms_gpu.py.

DRAW.  The row's uniform comes from Philox4x32-10 (step_dropout_model's, numpy uint64) at counter (env_offset + b, 0xFFFFFFFF,
step, episode mod 2^32) and key (seed mod 2^32, seed >> 32): u = float32(word0 >> 8) * 2^-24.  The pick is then
policy_head_model's sampling rule, restated here row by row.  GIVEN.  m and S as policy_head_model.row_weights computes them,
logp = (l[ptr] - m) - log S; NaN for a column outside [0, nR) or an unselectable one; probs as the sampling form's."""
import math

import numpy as np

import policy_head_model as HM
import step_dropout_model as SD

PICK_ROW = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def words(seed, episode, step, envs, row=PICK_ROW):
    """the four Philox output words for each env index of ``envs`` (already offset) -> 4 uint64 arrays of values < 2^32"""
    b = np.asarray(envs, np.uint64) & np.uint64(M32)
    zero = np.zeros_like(b)
    return SD.philox4x32_10((b, zero + np.uint64(row), zero + np.uint64(step & M32), zero + np.uint64(episode & M32)),
                            (seed & M32, (seed >> 32) & M32))


def uniforms(seed, episode, step, B, env_offset=0):
    """-> u (B,) float32 in [0, 1): (word0 >> 8) * 2^-24, both steps exact in fp32"""
    w0 = words(seed, episode, step, np.arange(B, dtype=np.uint64) + np.uint64(env_offset))[0]
    return (w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def draw_row(logits, mask, u):
    """one row of the DRAW form given its uniform -> (ptr, logp fp64, probs fp64 (nR,)): t = u S; the first selectable column
    whose inclusive prefix sum exceeds t, the last selectable one when none does; an empty row is (0, NaN, zeros)"""
    probs = np.zeros(len(mask), np.float64)
    sel, m, w, cum, S = HM.row_weights(logits, mask)
    if not sel:
        return 0, float('nan'), probs
    t = float(np.float32(u)) * S
    ptr = sel[-1]
    for i, c in enumerate(sel):
        if cum[i] > t:
            ptr = c
            break
    for i, c in enumerate(sel):
        probs[c] = w[i] / S
    return ptr, (float(logits[ptr]) - m) - math.log(S), probs


def draw(logits, mask, seed, episode, step, env_offset=0):
    """-> ptr (B,) int64, logp (B,) fp64, probs (B, nR) fp64, u (B,) float32"""
    B, nR = mask.shape
    u = uniforms(seed, episode, step, B, env_offset)
    ptr, logp, probs = np.zeros(B, np.int64), np.zeros(B, np.float64), np.zeros((B, nR), np.float64)
    for b in range(B):
        ptr[b], logp[b], probs[b] = draw_row(logits[b], mask[b], u[b])
    return ptr, logp, probs, u


def given_row(logits, mask, p):
    """-> (logp fp64, probs fp64 (nR,))"""
    nR = len(mask)
    probs = np.zeros(nR, np.float64)
    sel, m, w, _, S = HM.row_weights(logits, mask)
    for i, c in enumerate(sel):
        probs[c] = w[i] / S
    p = int(p)
    if not sel or not 0 <= p < nR or mask[p] == 0:
        return float('nan'), probs
    return (float(logits[p]) - m) - math.log(S), probs


def given(logits, mask, ptr):
    """-> logp (B,) fp64, probs (B, nR) fp64"""
    B, nR = mask.shape
    logp, probs = np.zeros(B, np.float64), np.zeros((B, nR), np.float64)
    for b in range(B):
        logp[b], probs[b] = given_row(logits[b], mask[b], ptr[b])
    return logp, probs


# ---- the shapes of the GPU comparison: every instantiation, the smallest sizes that reach it ---------------------------
DRAW_AT = ((0x5EED << 32) | 77, 3, 4, 9)     # (seed, episode, step, env_offset) of the fixed comparison
NR_LIST = [5, 12, 20, 40, 64, 65, 130]       # G = 8, 16, 32, 64, 64; the chunked form with a ragged and a third chunk


def batch_sizes(nR):
    """B = 1, one more row than a workgroup of 256 threads holds for this G, and 67: a ragged last wave"""
    G = HM.group_of(nR) or 64
    return [1, 256 // G + 1, 67]


def case(nR, B, seed=0):
    """-> logits, mask (B, nR) float32: randn * 3 at 40 % selectable, with -- where the batch has the rows -- row 0 fully
    selectable, row 1 with one selectable column and row 2 with none"""
    rng = np.random.RandomState(7000 + 100 * nR + B + 13 * seed)
    logits = (rng.randn(B, nR) * 3).astype(np.float32)
    mask = (rng.rand(B, nR) < 0.4).astype(np.float32)
    mask[0] = 1
    if B > 1:
        mask[1] = 0
        mask[1, nR // 2] = 1
    if B > 2:
        mask[2] = 0
    return logits, mask
