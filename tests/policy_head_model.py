"""The decoding head's semantics (tapenv.h: tap_policy_pick / tap_policy_pick_backward) restated sequentially in numpy
fp64: the oracle of tests/test_policy_head_cpu.py and tests/test_policy_head_gpu.py.  Row by row, column by column,
left to right; nothing here is vectorised across the columns, so the order of every sum is the obvious one."""
import math

import numpy as np

NR_LIST = [1, 2, 7, 8, 9, 16, 20, 33, 60, 64, 65, 120, 128, 256, 300]    # every G, both sides of each switch, the chunked form
SEEDS = [0, 1, 2, 3, 4]


def group_of(nR):
    """lanes per row of the device head: 0 = the chunked form"""
    return 8 if nR <= 8 else 16 if nR <= 16 else 32 if nR <= 32 else 64 if nR <= 64 else 0


def batch_sizes(nR):
    G = group_of(nR) or 64
    return [1, 3, 64 // G + 1, 257]


def row_weights(logits, mask):
    """-> (sel columns, m, w per selectable column (fp64), prefix sums (fp64), S); m = None on an empty row"""
    sel = [c for c in range(len(mask)) if mask[c] != 0]
    if not sel:
        return sel, None, [], [], 0.0
    m = max(float(logits[c]) for c in sel)
    w, cum, run = [], [], 0.0
    for c in sel:
        w.append(math.exp(float(logits[c]) - m))
        run += w[-1]
        cum.append(run)
    return sel, m, w, cum, run


def pick_row(logits, mask, u=None):
    """-> (ptr, logp fp64, probs fp64 (nR,), gap): gap = min |t - boundary| / S over the prefix sums the rule compares t
    with (inf for the greedy branch and an empty row)"""
    nR = len(mask)
    probs = np.zeros(nR, np.float64)
    sel, m, w, cum, S = row_weights(logits, mask)
    if not sel:
        return 0, float('nan'), probs, float('inf')
    gap = float('inf')
    if u is None:
        k = next(i for i, c in enumerate(sel) if float(logits[c]) == m)
    else:
        t = float(np.float32(u)) * S
        k = next((i for i in range(len(sel)) if cum[i] > t), len(sel) - 1)
        gap = min(abs(t - b) for b in cum) / S
    for i, c in enumerate(sel):
        probs[c] = w[i] / S
    ptr = sel[k]
    return ptr, (float(logits[ptr]) - m) - math.log(S), probs, gap


def pick(logits, mask, u=None):
    """batched pick_row -> ptr (B,) int64, logp (B,) fp64, probs (B, nR) fp64, gap (B,) fp64"""
    B, nR = mask.shape
    ptr = np.zeros(B, np.int64)
    logp = np.zeros(B, np.float64)
    probs = np.zeros((B, nR), np.float64)
    gap = np.zeros(B, np.float64)
    for b in range(B):
        ptr[b], logp[b], probs[b], gap[b] = pick_row(logits[b], mask[b], None if u is None else u[b])
    return ptr, logp, probs, gap


def backward(probs, ptr, logp, g):
    """dlogits (B, nR) fp64 from fp64 probs: g * (onehot(ptr) - probs), zero rows where logp is NaN"""
    B, nR = probs.shape
    out = np.zeros((B, nR), np.float64)
    for b in range(B):
        if math.isnan(logp[b]):
            continue
        for c in range(nR):
            out[b, c] = float(g[b]) * ((1.0 if c == ptr[b] else 0.0) - probs[b, c])
    return out


# ---- the fixed inputs of the GPU comparison (the CPU test checks their distance from every prefix sum) ---------------
# (logits kind, mask density): randn * 3 at c2's live share (13 %), at 30 % and fully selectable; magnitudes +-80 (no
# path without the max subtraction survives them in fp32); all-equal logits
COMBOS = [("randn", 0.3), ("randn", 1.0), ("randn", 0.13), ("big", 0.3), ("equal", 0.3)]
MIN_GAP = 1e-9        # every u * S of the fixed cases stays this far (times S) from every prefix sum


def sample_case(nR, B, kind, density, seed):
    """-> logits (B, nR) f32, mask (B, nR) f32 of 0 / 1 (rows may come out empty: the empty-row rule), u (B,) f32"""
    rng = np.random.RandomState(100000 * seed + 100 * nR + COMBOS.index((kind, density)))
    if kind == "randn":
        logits = rng.randn(B, nR) * 3
    elif kind == "big":
        logits = rng.choice([-80.0, 80.0], size=(B, nR)) + rng.randn(B, nR)
    else:
        logits = np.full((B, nR), 1.5)
    mask = (rng.rand(B, nR) < density).astype(np.float32)
    u = rng.rand(B).astype(np.float32)
    return logits.astype(np.float32), mask, u


def fixed_cases(nR):
    """the (nR, B, kind, density, seed) of the GPU comparison for one nR"""
    out = []
    for i, B in enumerate(batch_sizes(nR)):
        for j, (kind, density) in enumerate(COMBOS):
            out.append((nR, B, kind, density, SEEDS[(i + j) % len(SEEDS)]))
    return out


_REF = {}


def reference(case, greedy):
    """pick() of a fixed case, computed once per process"""
    key = (case, bool(greedy))
    if key not in _REF:
        logits, mask, u = sample_case(*case)
        _REF[key] = pick(logits, mask, None if greedy else u)
    return _REF[key]


def neighbour32(got, want64):
    """got (fp32 array) is the fp64 value rounded to fp32 or one of that value's two fp32 neighbours; NaN matches NaN"""
    want = np.asarray(want64, np.float64).astype(np.float32)
    got = np.asarray(got, np.float32)
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    same_nan = np.isnan(got) & np.isnan(want)
    return same_nan | (got == want) | (got == lo) | (got == hi)
