"""The numpy model of the dynamic encoder on the bit shadow (tapenv.h: tap_encode_bits): unpack the shadow, then the
sequential fp32 sum in ascending row order -- the order the contract fixes, so the device must give these bytes -- and
the float64 sums the backward is held to."""
import numpy as np

U32 = 2.0 ** -24            # the unit roundoff of fp32


def planes_of(rows):
    return 2 if rows > 64 else 1


def pack_bits(dyn):
    """(B, rows, nR) 0/1 array -> the shadow (B, planes * nR) int64 in pack.dynamic_bits layout"""
    B, rows, nR = dyn.shape
    P = planes_of(rows)
    out = np.zeros((B, P, nR), np.uint64)
    for r in range(rows):
        out[:, r // 64, :] |= (dyn[:, r, :] != 0).astype(np.uint64) << np.uint64(r % 64)
    return out.reshape(B, P * nR).view(np.int64)


def unpack_bits(bits, rows, nR):
    """the shadow -> (B, rows, nR) bool; bits at positions >= rows are ignored"""
    B = bits.shape[0]
    w = np.ascontiguousarray(bits).reshape(B, planes_of(rows), nR).view(np.uint64)
    out = np.empty((B, rows, nR), bool)
    for r in range(rows):
        out[:, r, :] = ((w[:, r // 64, :] >> np.uint64(r % 64)) & np.uint64(1)) != 0
    return out


def garbage(bits, rows, nR, seed):
    """the same shadow with random bits at the positions >= rows (which the encoder must ignore)"""
    B = bits.shape[0]
    P = planes_of(rows)
    w = np.ascontiguousarray(bits).reshape(B, P, nR).view(np.uint64).copy()
    rng = np.random.RandomState(seed)
    junk = rng.randint(0, 2 ** 32, size=w.shape, dtype=np.uint64) << np.uint64(32) | rng.randint(0, 2 ** 32, size=w.shape, dtype=np.uint64)
    for p in range(P):
        used = min(64, rows - 64 * p)
        keep = np.uint64((1 << used) - 1) if used < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
        w[:, p, :] = (w[:, p, :] & keep) | (junk[:, p, :] & ~keep)
    return w.reshape(B, P * nR).view(np.int64)


def encode(bits, weight, bias, rows, nR):
    """out (B, H, nR) float32: starts at bias[h] (+0.0 without one), then one fp32 addition per row r in ascending
    order: W[h, r] where the bit is set, +0.0 where it is not"""
    dyn = unpack_bits(bits, rows, nR)
    W = np.asarray(weight, np.float32)
    B, H = dyn.shape[0], W.shape[0]
    acc = np.zeros((B, H, nR), np.float32)
    if bias is not None:
        acc += np.asarray(bias, np.float32)[None, :, None]
    zero = np.float32(0.0)
    for r in range(rows):
        acc = acc + np.where(dyn[:, r, :][:, None, :], W[:, r][None, :, None], zero)
    assert acc.dtype == np.float32
    return acc


def encode64(dyn, weight, bias):
    """the float64 value of the same convolution, and sum |terms| per output (for the error bound)"""
    d = dyn.astype(np.float64)
    W = np.asarray(weight, np.float64)
    out = np.einsum('hr,brc->bhc', W, d)
    mag = np.einsum('hr,brc->bhc', np.abs(W), d)
    if bias is not None:
        out = out + np.asarray(bias, np.float64)[None, :, None]
        mag = mag + np.abs(np.asarray(bias, np.float64))[None, :, None]
    return out, mag


def backward64(bits, g, rows, nR):
    """float64 dweight (H, rows), dbias (H,), and the sums of |terms| of each (for K * 2^-24 * sum |terms|)"""
    d = unpack_bits(bits, rows, nR).astype(np.float64)
    g64 = np.asarray(g, np.float64)
    dW = np.einsum('bhc,brc->hr', g64, d)
    dWm = np.einsum('bhc,brc->hr', np.abs(g64), d)
    return dW, g64.sum(axis=(0, 2)), dWm, np.abs(g64).sum(axis=(0, 2))


def random_case(B, rows, nR, H, density, seed, bias=True, spiky=True):
    """bits at ``density``, randn weights with (``spiky``) one hidden row of huge / tiny magnitudes of mixed sign, so
    that a sum taken in another order gives other bytes"""
    rng = np.random.RandomState(seed)
    dyn = rng.rand(B, rows, nR) < density
    W = rng.randn(H, rows).astype(np.float32)
    if spiky:
        h = H // 2
        mags = np.array([1e30, -1e30, 1e-30, 3.0, -1e30, 1e30, -7.0], np.float32)
        W[h, :] = mags[np.arange(rows) % len(mags)] * (1 + rng.rand(rows).astype(np.float32) * (np.arange(rows) % 7 >= 2))
    b = rng.randn(H).astype(np.float32) if bias else None
    return dyn, pack_bits(dyn), W, b
