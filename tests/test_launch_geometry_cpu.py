"""The launch geometry that pointer.hip and encode.hip choose from the batch size, through the host-only queries
tap_pointer_scores_geometry / tap_encode_bits_geometry (tapenv.h): no GPU.  The queries are answered by the function the
launcher itself calls, so (1) they must agree with what the scratch-size queries already show of the same geometry, over a
seeded sweep of the supported domain, and (2) the shapes that tests/test_launch_geometry_gpu.py runs
(tests/launch_geometry_cases.py) must reach, by the library's own answer, every class they are there for: a change of the
launcher's rule or of the list that loses one fails here."""
import ctypes as C

import numpy as np
import pytest

import launch_geometry_cases as LG
from tap_net_amd import _lib

LDS_BUDGET = 60 * 1024


def _ptr(B, nR, rows, Hd, S, backward):
    return _lib.pointer_scores_geometry(B, nR, rows, Hd, S, backward)


def _unhalved(B):
    """envs per workgroup that a batch asks for, from the library: the lightest shape's answer (its LDS never binds)"""
    epb, _, lds, _ = _ptr(B, 4, 1, 64, 0, False)
    assert lds < LDS_BUDGET // 2
    return epb


_BATCH_OF = {}


def _batch_of(e):
    """a batch that asks for ``e`` envs per workgroup, found by asking the library"""
    if not _BATCH_OF:
        for b in [1024 * m for m in range(17, 0, -1)] + [1]:               # the sweep's batches ask for 16 at the most
            _BATCH_OF[_unhalved(b)] = b
    return _BATCH_OF[e]


def _batches(rng):
    edge = sorted({b for m in range(1024, 16400 + 1, 1024) for b in (m - 1, m, m + 1)} | {1, 2, 1023, 16400})
    return edge + [int(b) for b in rng.randint(1, 16401, size=40)]


def test_pointer_query_agrees_with_the_scratch_queries():
    L, rng = _lib.lib(), np.random.RandomState(20261)
    seen_halved, seen_epb = 0, set()
    for B in _batches(rng):
        for _ in range(6):
            rows, nR, Hd, S = int(rng.randint(1, 129)), 4 * int(rng.randint(1, 65)), int(rng.choice([64, 128, 256])), int(rng.randint(0, 9))
            for backward in (False, True):
                epb, blocks, lds, ct = _ptr(B, nR, rows, Hd, S, backward)
                assert 1 <= epb <= _unhalved(B) and blocks == -(-B // epb) and 0 < lds <= LDS_BUDGET, (B, nR, rows, Hd, S, backward)
                hck = 128 if rows <= 64 and Hd > 64 else 64
                assert ct == (min(nR, 4096 // hck) if backward else 0)
                seen_epb.add(epb)
                seen_halved += epb < _unhalved(B)
                e = _unhalved(B)
                while e > epb:                                             # reached by halving, and every count before it did not fit
                    assert _ptr(_batch_of(e), nR, rows, Hd, S, backward)[0] < e, (B, nR, rows, Hd, S, backward, e)
                    e >>= 1
                assert e == epb
            need = L.tap_pointer_scores_static_backward_scratch(B, nR, rows, Hd, S) if S else L.tap_pointer_scores_backward_scratch(B, nR, rows, Hd)
            assert need == blocks * 2 * Hd * 4, (B, nR, rows, Hd, S)
    assert seen_halved > 50 and seen_epb >= set(range(1, 9))


def test_encoder_query_agrees_with_the_scratch_query():
    L, rng = _lib.lib(), np.random.RandomState(20262)
    for B in _batches(rng):
        for _ in range(6):
            rows, nR, H = int(rng.randint(1, 129)), 4 * int(rng.randint(1, 65)), int(rng.randint(1, 1025))
            epb, gx, gy, lds = _lib.encode_bits_geometry(B, nR, rows, H, False)
            hck = 128 if rows <= 64 and H > 64 else 64
            assert 1 <= epb <= B and gx == -(-B // epb) and gy == -(-H // hck) and 0 < lds <= LDS_BUDGET, (B, nR, rows, H)
            per, slices, chunks, hc = _lib.encode_bits_geometry(B, nR, rows, H, True)
            assert per >= 1 and slices == -(-B // per) and 1 <= hc <= H and chunks == -(-H // hc), (B, nR, rows, H)
            assert slices * chunks <= 1024 and hc * nR <= 8192 and hc * (rows + 1) <= 16 * 256   # the partials, the kernel's LDS tile and registers
            assert L.tap_encode_bits_backward_scratch(B, nR, rows, H) == slices * H * (rows + 1) * 4, (B, nR, rows, H)


def test_refused_shapes_answer_zeros():
    L = _lib.lib()
    out = (C.c_int32 * 4)(7, 7, 7, 7)
    inv, uns = _lib.TAP_E_INVALID, _lib.TAP_E_UNSUPPORTED
    for args, want in (((0, 20, 30, 128, 0, 0), inv), ((8, 0, 30, 128, 0, 1), inv), ((8, 20, 30, 128, -1, 0), inv),
                       ((8, 22, 30, 128, 0, 0), uns), ((8, 20, 129, 128, 2, 1), uns), ((8, 20, 30, 96, 0, 0), uns),
                       ((8, 20, 30, 128, 9, 1), uns), ((8, 260, 30, 128, 0, 0), uns)):
        out[:] = [7, 7, 7, 7]
        assert L.tap_pointer_scores_geometry(*args, out) == want and list(out) == [0, 0, 0, 0], args
        B, nR, rows, Hd, S = args[:5]
        if S >= 0:
            assert (L.tap_pointer_scores_static_backward_scratch(B, nR, rows, Hd, S) if S else L.tap_pointer_scores_backward_scratch(B, nR, rows, Hd)) == 0
    for args, want in (((0, 20, 30, 128, 0), inv), ((8, 20, 0, 128, 1), inv), ((8, 22, 30, 128, 0), uns), ((8, 20, 30, 1025, 1), uns),
                       ((8, 20, 129, 7, 0), uns)):
        out[:] = [7, 7, 7, 7]
        assert L.tap_encode_bits_geometry(*args, out) == want and list(out) == [0, 0, 0, 0], args
        assert L.tap_encode_bits_backward_scratch(*args[:4]) == 0
    assert L.tap_pointer_scores_geometry(8, 20, 30, 128, 0, 0, None) == inv and L.tap_encode_bits_geometry(8, 20, 30, 128, 0, None) == inv
    with pytest.raises(_lib.TapError):
        _lib.pointer_scores_geometry(8, 20, 30, 96)
    with pytest.raises(_lib.TapError):
        _lib.encode_bits_geometry(8, 22, 30, 7)


def _classes(cases, backward):
    """per form (S) the set of (before, after, shape) that the library gives the list's shapes; each case's own claim checked"""
    out = {}
    for B, nR, rows, Hd, S, (before, after) in cases:
        epb, blocks, lds, _ = _ptr(B, nR, rows, Hd, S, backward)
        assert (_unhalved(B), epb) == (before, after), ((B, nR, rows, Hd, S), _unhalved(B), epb)
        assert B % 1024 in (2, 3)
        assert (epb == 1 or B % epb != 0) and blocks > 2                   # a ragged last workgroup, and a middle one
        assert max(B * 3 * Hd * nR * 4, 1) <= (800 << 20)                  # proj / dU: under 0.8 GB
        assert 3 * max(after, B - (blocks - 1) * after) <= 64              # the sample: three workgroups' envs, at most 64
        out.setdefault(S, set()).add((before, after, nR, rows, Hd))
    return out


def test_pointer_forward_cases_reach_every_class():
    by_form = _classes(LG.POINTER_FW, False)
    assert set(by_form) == {0, 2, 5}
    for S in (0, 2):
        got = by_form[S]
        assert {(b, a) for b, a, *_ in got} >= {(3, 3), (4, 4), (5, 5), (8, 8), (10, 5), (12, 6)}, S
        at8 = {(nR, rows, Hd) for b, a, nR, rows, Hd in got if (b, a) == (8, 8)}
        assert (20, 30, 128) in at8 and (60, 30, 128) in at8               # the benchmark's geometry and its 3D window
        assert any(nR > 64 for nR, _, _ in at8)                            # several columns per lane in the softmax
        assert any(rows > 64 for _, rows, _ in at8)                        # two shadow planes
        assert any(a > LG.POINTER_NW and a % LG.POINTER_NW for _, a, *_ in got)     # a second, partial round of the softmax loop
        assert any(a == 2 * LG.POINTER_NW for _, a, *_ in got)             # and a second full one
        assert any(a % 2 for _, a, *_ in got if a > 2) and any(b > a and a % 2 for b, a, *_ in got)   # odd counts, one from halving
    assert {(b, a) for b, a, *_ in by_form[5]} == {(8, 8), (9, 4)}         # the LDS copy of G: at 8, and what it costs 9
    # the same shape without the copy is not halved: it is G's copy that halves it
    assert _ptr(9219, 4, 64, 256, 2, False)[0] == 9 and _ptr(9219, 4, 64, 256, 0, False)[0] == 9


def test_pointer_backward_cases_reach_every_class():
    by_form = _classes(LG.POINTER_BW, True)
    assert set(by_form) == {0, 2, 5}
    for S in (0, 2):
        got = {(b, a) for b, a, *_ in by_form[S]}
        assert got >= {(3, 3), (8, 8), (5, 5), (3, 1), (4, 2), (6, 3), (8, 4)}, (S, got)
    assert {(b, a) for b, a, *_ in by_form[5]} == {(2, 1)} and _ptr(2051, 100, 64, 256, 2, True)[0] == 2
    # the reduce's second level: more than one run of 32 partials, with a last run that is not full
    for B, nR, rows, Hd, S, _ in LG.POINTER_BW:
        blocks = _ptr(B, nR, rows, Hd, S, True)[1]
        assert blocks > LG.REDUCE_RUN and blocks % LG.REDUCE_RUN
    # several passes of the dU tile (nR above the columns per pass) among the halved ones
    assert any(_ptr(B, nR, rows, Hd, S, True)[3] < nR for B, nR, rows, Hd, S, _ in LG.POINTER_BW)
    assert {c[:4] for c in LG.POINTER_BW if c[1] == 4} == {(5123, 4, 10, 64), (8195, 4, 64, 256)}    # where the batch sums are checked


def test_encoder_and_critic_cases_reach_every_class():
    L = _lib.lib()
    assert {_lib.encode_bits_geometry(B, nR, rows, H, False)[0] for B, nR, rows, H in LG.ENCODER_FW} == {3, 8}
    for want in (3, 8):                                                    # each with a ragged last workgroup
        assert any(_lib.encode_bits_geometry(B, nR, rows, H, False)[0] == want and B % want for B, nR, rows, H in LG.ENCODER_FW)
    bw = [_lib.encode_bits_geometry(B, nR, rows, H, True) for B, nR, rows, H in LG.ENCODER_BW]
    assert bw[0][0] == 9 and bw[0][2] == 1                                 # 9 envs per slice at the benchmark's batch
    assert bw[1][0] > 3 and bw[1][2] > 1 and LG.ENCODER_BW[1][0] >= 4099   # several hidden chunks, more envs per slice than before
    assert all(B % per for (B, _, _, _), (per, _, _, _) in zip(LG.ENCODER_BW, bw))   # a ragged last slice
    # the critic's workgroups, from its scratch (dU resident: the partials alone, one row of H floats per workgroup)
    blocks = [L.tap_critic_value_backward_scratch(B, nR, rows, H, S, n) // (4 * H) for rows, nR, H, S, n, B in LG.CRITIC_BW]
    assert blocks == [-(-c[5] // 4) for c in LG.CRITIC_BW] == [33, 1025]
    assert LG.REDUCE_RUN < blocks[0] < 2 * LG.REDUCE_RUN                   # the second run is entered, and is short
    assert [c[5] for c in LG.CRITIC_FW] == [4099] and all(c[5] % 4 for c in LG.CRITIC_FW + LG.CRITIC_BW)
