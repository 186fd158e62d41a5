"""MACS / MUL whole episodes on containers above the lane-per-cell kernels (2D: more than 64 columns; 3D: more than 64
cells or a side above 8) in ONE launch: k_macs2d_wave_episode (macs_big.hip) and k_macs3d_wave_episode (macs3_big.hip),
one wavefront per container with its tile resident in LDS across the placements.  Through the C ABI (tap_pack_blocks,
tap_episode_scores) against the CPU oracle and against the stepped path of the same library (pack._stepped_scores: n
placement launches on a state blob), and through pack.episode_scores / pack.render.  Before these kernels every call
here returned TAP_E_UNSUPPORTED and the Python layer stepped."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import oracle_lib as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _blocks(rs, B, n, D, lo, hi, hlo=1, hhi=6):
    b = rs.randint(lo, hi, size=(B, n, D)).astype(np.int32)
    b[:, :, -1] = rs.randint(hlo, hhi, size=(B, n))
    return b


# (container, block sides [lo, hi), reward type, B, n); the odd batch sizes leave the last workgroup ragged
CASES = [([65, 60], (8, 31), "C+P+S-mcs-soft", 33, 12),
         ([100, 60], (10, 46), "C+P+S-mul-soft", 17, 12),
         ([130, 60], (10, 61), "C+P+S-mcs-hard", 19, 12),
         ([200, 60], (20, 91), "mcs-soft", 9, 12),                      # the zero-mode flag, (C+P) S ratio
         ([4096, 60], (300, 1501), "C+P+S-mul-hard", 5, 10),            # the largest 2D tile
         ([9, 7, 60], (2, 7), "C+P+S-mcs-soft", 33, 10),                # 63 cells, big only by its side
         ([10, 10, 60], (2, 8), "C+P+S-mul-soft", 17, 12),
         ([20, 20, 60], (3, 9), "mcs-soft", 9, 12),
         ([64, 64, 40], (8, 9), "C+P+S-mul-hard", 5, 10),               # the largest 3D tile
         ([12, 5, 200], (2, 6), "C+P+S-mcs-soft", 19, 14)]              # the second 64-bit word of the free-list grid
_IDS = ["x".join(map(str, c[0])) + "-" + c[2] for c in CASES]


def _case_blocks(cfg):
    cs, (lo, hi), _, B, n = cfg
    if cs == [12, 5, 200]:
        return _blocks(np.random.RandomState(5), B, n, 3, lo, hi, 10, 31)
    return _blocks(np.random.RandomState(cs[0] * 7 + cs[1] + n), B, n, len(cs), lo, hi)


def _oracle(cs, reward, blocks):
    """positions / stable / errs of O.run_episodes plus calc_positions_mcs's own `ratio` (no division) and five scores"""
    blocks = np.ascontiguousarray(blocks, dtype=np.int32)
    B, n, _ = blocks.shape
    ref = O.run_episodes(O.make_desc(cs, n, reward, "full", "MACS"), blocks, nthreads=8, want_features=False, want_heightmaps=False)
    ratio, scores = np.zeros(B, np.float64), np.zeros((B, 5), np.int64)
    for b in range(B):
        _, _, _, ratio[b], scores[b] = O.calc_positions_mcs(blocks[b], cs, reward)
    return dict(positions=ref["positions"], stable=ref["stable"], errs=ref["errs"], nerr=ref["nerr"], ratio=ratio, scores=scores)


@functools.lru_cache(maxsize=None)
def _case_ref(i):
    """the oracle on a case's blocks, computed once and shared (read-only)"""
    cfg = CASES[i]
    return _oracle(cfg[0], cfg[2], _case_blocks(cfg))


def _wave_kind(L, D):
    return L.TAP_HIT_EPISODE_MACS2_WAVE if D == 2 else L.TAP_HIT_EPISODE_MACS3_WAVE


def _hits(L, kinds):
    return {k: v for k, v in L.variant_hits(DEV).items() if k[0] in kinds}


def _lane_kinds(L):
    return (L.TAP_HIT_EPISODE_MACS2, L.TAP_HIT_EPISODE_MACS3)


def _pack_blocks(L, cs, n, reward, blocks):
    """tap_pack_blocks with a MACS descriptor -> (status, positions, stable, reward fp32, score fp64); the outputs are
    pre-filled so that slots the kernel must zero show"""
    B, D = blocks.shape[0], len(cs)
    desc = L.make_desc(B, cs, n, reward, "full", "MACS")
    bt = torch.as_tensor(np.ascontiguousarray(blocks, dtype=np.int32), device=DEV)
    pos = torch.full((B, n, D), -7, dtype=torch.int32, device=DEV)
    st = torch.full((B, n), 9, dtype=torch.uint8, device=DEV)
    rew = torch.full((B,), 123.0, dtype=torch.float32, device=DEV)
    s64 = torch.full((B,), 123.0, dtype=torch.float64, device=DEV)
    c = L.ctx(DEV)
    with torch.cuda.device(DEV):
        rc = L.lib().tap_pack_blocks(c, C.byref(desc), B, n, L.ptr(bt), L.ptr(rew), L.ptr(pos), L.ptr(st), L.ptr(s64), L.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, pos.cpu().numpy(), st.cpu().numpy(), rew.cpu().numpy(), s64.cpu().numpy()


def _episode_scores(L, cs, n, reward, static, tour, target=-1):
    """tap_episode_scores -> (status, ratio, scores, err)"""
    B, rows, nR = static.shape
    desc = L.make_desc(B, cs, n, reward, "full", "MACS")
    ratio = torch.full((B,), 123.0, dtype=torch.float64, device=DEV)
    scores = torch.full((B, 5), -7, dtype=torch.int64, device=DEV)
    err = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    c = L.ctx(DEV)
    with torch.cuda.device(DEV):
        rc = L.lib().tap_episode_scores(c, C.byref(desc), B, n, L.ptr(static), rows, nR, L.ptr(tour), target, L.ptr(ratio), L.ptr(scores),
                                        None, None, L.ptr(err), L.stream_of(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, ratio.cpu().numpy(), scores.cpu().numpy(), err.cpu().numpy()


def _static_of(blocks, ids=None):
    """static in PACKDataset's layout (row 0 = block id, column r * n + i = block i in rotation r) [+ a target-id row]"""
    B, n, D = blocks.shape
    perms = list(itertools.permutations(range(D)))
    R = len(perms)
    static = torch.zeros(B, 1 + D + (ids is not None), n * R, device=DEV)
    static[:, 0] = torch.arange(n, device=DEV).repeat(R)
    bf = torch.as_tensor(blocks, device=DEV, dtype=torch.float32)
    for r, perm in enumerate(perms):
        for k in range(D):
            static[:, 1 + k, r * n:(r + 1) * n] = bf[:, :, perm[k]]
    if ids is not None:
        static[:, -1] = torch.as_tensor(ids, device=DEV, dtype=torch.float32).repeat(1, R)
    return static.contiguous(), R


def _gather(static, tour, D):
    stn, tn = static.cpu().numpy(), tour.cpu().numpy()
    B, n = tn.shape
    return np.stack([stn[np.arange(B), 1:1 + D, tn[:, t]] for t in range(n)], axis=1).astype(np.int32)


def _stepped_errors(T, cs, n, reward, static, tour):
    """the sticky error words of the same episode stepped on a state blob (what pack._stepped_scores runs)"""
    env = T.BatchedContainer(static.shape[0], cs, n, reward, "full", packing_strategy="MACS", device=DEV)
    for t in range(n):
        env.add_new_blocks_gather(static, tour[:, t].contiguous(), want_feature=False)
    return env.errors.cpu().numpy()


def _same_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("i", range(len(CASES)), ids=_IDS)
def test_one_launch_episodes(T, i):
    """tap_pack_blocks against the oracle (every container: the cases raise no error and stack blocks), tap_episode_scores
    on tours against the stepped path (every container, errors included) and the oracle, one launch of the new kind each.

    The tours: PACKDataset's static holds every rotation of a block, and a rotation that turns a block's height into a
    side can overflow H or exceed the container -- the reference raises there.  Containers with an even index draw
    their tour from the unrotated columns only (the case's own blocks in another order: no error), the others from all
    n R columns, so both the plain and the flagged outcomes are compared with the stepped path."""
    from tap_net_amd import _lib as L, pack
    cs, _, reward, B, n = CASES[i]
    D = len(cs)
    blocks = _case_blocks(CASES[i])
    want = _case_ref(i)
    assert want["nerr"] == 0
    if cs == [12, 5, 200]:
        assert want["positions"][..., 2].max() >= 64                              # the second word of the free-list grid is in use
    if cs != [64, 64, 40]:                       # (ten 8 x 8 blocks all find room on that floor: the case is the largest tile)
        assert int((want["positions"][..., -1] > 0).sum()) >= 27                  # blocks are stacked, not laid side by side

    # 1. explicit block lists
    L.variant_hits_reset(DEV)
    rc, pos, st, rew, s64 = _pack_blocks(L, cs, n, reward, blocks)
    assert rc == L.TAP_OK, rc                                                     # TAP_E_UNSUPPORTED before the wave-episode kernels
    assert np.array_equal(pos, want["positions"])
    assert np.array_equal(st, want["stable"])
    assert np.array_equal(_bits(s64), _bits(want["ratio"]))
    assert np.array_equal(rew, -want["ratio"].astype(np.float32))
    # 3. one launch of the new kind, none of the lane-per-cell episode kernels
    hits = _hits(L, (_wave_kind(L, D),) + _lane_kinds(L))
    assert list(hits.values()) == [1] and next(iter(hits))[:3] == (_wave_kind(L, D), D, 64), hits
    assert 1 <= next(iter(hits))[5] <= 4 and next(iter(hits))[3:5] == (0, 0) and next(iter(hits))[6] == 0

    # 2. static + tour
    static, R = _static_of(blocks)
    g = torch.Generator().manual_seed(7)
    tour = torch.stack([torch.randperm(n if b % 2 == 0 else n * R, generator=g)[:n] for b in range(B)]).to(DEV)
    L.variant_hits_reset(DEV)
    rc, ratio, scores, err = _episode_scores(L, cs, n, reward, static, tour)
    assert rc == L.TAP_OK, rc
    hits = _hits(L, (_wave_kind(L, D),) + _lane_kinds(L))
    assert list(hits.values()) == [1] and next(iter(hits))[0] == _wave_kind(L, D), hits
    r_s, s_s = pack._stepped_scores(static, tour, cs, n, reward, "MACS", None, check=False)
    r_s, s_s = r_s.cpu().numpy(), s_s.cpu().numpy()
    assert _same_f64(ratio, r_s)
    assert np.array_equal(scores, s_s)
    assert np.array_equal(err, _stepped_errors(T, cs, n, reward, static, tour))   # the error words are the stepped path's, bit for bit
    assert np.array_equal(err != 0, np.isnan(r_s))
    w2 = _oracle(cs, reward, _gather(static, tour, D))
    good = w2["errs"] == 0
    assert good[0::2].all() and good.sum() >= (B + 1) // 2
    print("%s: %d of %d tours without an error" % (_IDS[i], int(good.sum()), B))
    assert np.array_equal(err != 0, ~good)
    assert np.array_equal(_bits(ratio[good]), _bits(w2["ratio"][good]))
    assert np.array_equal(scores[good], w2["scores"][good])
    assert np.isnan(ratio[~good]).all()


@pytest.mark.parametrize("cs,lo,hi", [([100, 60], 10, 46), ([10, 10, 60], 2, 8)], ids=["100x60", "10x10x60"])
def test_target_lists(T, cs, lo, hi):
    """the two-container input types: target = 0 | 1 packs the entries with that id; an empty list scores zeros"""
    from tap_net_amd import _lib as L, pack
    B, n, D, reward = 11, 10, len(cs), "C+P+S-mcs-soft"
    rs = np.random.RandomState(31 + D)
    blocks = _blocks(rs, B, n, D, lo, hi)
    ids = rs.randint(0, 2, size=(B, n))
    ids[0, :2] = (0, 1)                                                           # both ids present in the row
    ids[3] = 0                                                                    # container 3: every entry has id 0
    static, R = _static_of(blocks, ids)
    tour = torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(b)) for b in range(B)]).to(DEV)
    for target in (0, 1):
        L.variant_hits_reset(DEV)
        ratio, scores = pack.episode_scores(static, tour, reward, "mul", True, cs, "MACS", target=target, check=False)
        hits = _hits(L, (_wave_kind(L, D),) + _lane_kinds(L))
        assert list(hits.values()) == [1] and next(iter(hits))[0] == _wave_kind(L, D), hits
        r_s, s_s = pack._stepped_scores(static, tour, cs, n, reward, "MACS", target, check=False)
        assert np.array_equal(_bits(ratio.cpu().numpy()), _bits(r_s.cpu().numpy()))
        assert torch.equal(scores, s_s)
        assert not torch.isnan(ratio).any()
        bl = _gather(static, tour, D)
        tn = tour.cpu().numpy()
        for b in (0, 3, B - 1):                                                   # and the oracle on the sub-list
            mine = bl[b][ids[b][tn[b]] == target]
            if len(mine):
                rc, _, _, want_r, want_s = O.calc_positions_mcs(mine, cs, reward)
                assert rc == 0
            else:
                want_r, want_s = 0.0, np.zeros(5, np.int64)
            assert _bits(ratio[b].item()) == _bits(want_r) and np.array_equal(scores[b].cpu().numpy(), want_s), (target, b)
    assert ratio[3].item() == 0.0 and scores[3].tolist() == [0, 0, 0, 0, 0]        # target 1 of container 3: the empty list


@pytest.mark.parametrize("cs,lo,hi", [([100, 60], 10, 46), ([10, 10, 60], 2, 8)], ids=["100x60", "10x10x60"])
def test_pack_blocks_skips_entries_with_a_zero_side(T, cs, lo, hi):
    """a side < 1 marks "not in this list": zero output slots, the rest as the compacted list"""
    from tap_net_amd import _lib as L
    B, n, D, reward = 7, 9, len(cs), "C+P+S-mul-soft"
    blocks = _blocks(np.random.RandomState(17 + D), B, n, D, lo, hi)
    blocks[:, 2, 0] = 0
    blocks[:, 6] = 0
    keep = [t for t in range(n) if t not in (2, 6)]
    want = _oracle(cs, reward, blocks[:, keep])
    assert want["nerr"] == 0
    rc, pos, st, rew, s64 = _pack_blocks(L, cs, n, reward, blocks)
    assert rc == L.TAP_OK, rc
    assert not pos[:, (2, 6)].any() and not st[:, (2, 6)].any()
    assert np.array_equal(pos[:, keep], want["positions"]) and np.array_equal(st[:, keep], want["stable"])
    assert np.array_equal(_bits(s64), _bits(want["ratio"]))
    assert np.array_equal(rew, -want["ratio"].astype(np.float32))


@pytest.mark.parametrize("cs,lo,hi", [([100, 12], 10, 31), ([10, 10, 12], 2, 5)], ids=["100x12", "10x10x12"])
def test_error_words(T, cs, lo, hi):
    """a block higher than the container (bit 1) and a tour index of nR (bit 4): flagged in exactly those containers,
    their ratio NaN, the others as the oracle; check=True raises like the reference's IndexError"""
    from tap_net_amd import _lib as L, pack
    B, n, D, reward = 5, 4, len(cs), "C+P+S-mcs-soft"
    blocks = _blocks(np.random.RandomState(3 + D), B, n, D, lo, hi, 1, 3)
    blocks[1, 2, -1] = 20                                                         # z + h > H = 12
    static, R = _static_of(blocks)
    nR = n * R
    tour = torch.arange(n, device=DEV).repeat(B, 1)
    tour[3, 1] = nR                                                               # the reference's gather raises
    rc, ratio, scores, err = _episode_scores(L, cs, n, reward, static, tour)
    assert rc == L.TAP_OK, rc
    assert err[1] == 1 and err[3] == 4 and not err[[0, 2, 4]].any(), err
    assert np.isnan(ratio[[1, 3]]).all()
    ok = [0, 2, 4]
    want = _oracle(cs, reward, blocks[ok])
    assert want["nerr"] == 0
    assert np.array_equal(_bits(ratio[ok]), _bits(want["ratio"])) and np.array_equal(scores[ok], want["scores"])
    r_s, s_s = pack._stepped_scores(static, tour, cs, n, reward, "MACS", None, check=False)
    assert _same_f64(ratio, r_s.cpu().numpy()) and np.array_equal(scores, s_s.cpu().numpy())
    assert np.array_equal(err, _stepped_errors(T, cs, n, reward, static, tour))
    with pytest.raises(L.TapOverflowError):
        pack.episode_scores(static, tour, reward, "bot", True, cs, "MACS", check=True)


@pytest.mark.parametrize("cs,lo,hi", [([100, 60], 10, 46), ([10, 10, 60], 2, 8)], ids=["100x60", "10x10x60"])
def test_render_takes_the_one_launch_path(T, tmp_path, cs, lo, hi):
    """pack.render with packing_strategy='MACS': the metric files hold the oracle's figures, from one launch"""
    from tap_net_amd import _lib as L
    B, n, D, reward = 13, 10, len(cs), "C+P+S-mcs-soft"
    blocks = _blocks(np.random.RandomState(41 + D), B, n, D, lo, hi)
    static, R = _static_of(blocks)
    tour = torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(50 + b)) for b in range(B)]).to(DEV)
    want_r, want_s, errs = O.render_scores(static.cpu().numpy(), tour.cpu().numpy(), reward, "bot", True, cs[0], cs[-1], "MACS",
                                           initial_container_height=cs[-1])
    assert not errs.any()
    L.variant_hits_reset(DEV)
    T.render(static, tour, str(tmp_path / "batch0_-1.2345.png"), None, 0.5, input_type="bot", allow_rot=True, container_width=cs[0],
             container_height=cs[-1], initial_container_width=7, initial_container_height=cs[-1], unit=1.0, packing_strategy="MACS",
             reward_type=reward)
    hits = _hits(L, (_wave_kind(L, D),) + _lane_kinds(L))
    assert list(hits.values()) == [1] and next(iter(hits))[0] == _wave_kind(L, D), hits
    assert np.array_equal(_bits(np.loadtxt(str(tmp_path / "batch-ratio.txt"))), _bits(want_r))
    for k, name in enumerate(("valid_size", "box_size", "empty_size", "stable_num", "packing_height")):
        assert np.array_equal(np.loadtxt(str(tmp_path / ("batch-%s.txt" % name))), want_s[:, k]), name


def test_size_boundaries(T):
    """65 columns, a 3D side of 9 and 72 cells go through the wave-episode kernels; 64 columns and 8 x 8 stay with the
    lane-per-cell episode kernels"""
    from tap_net_amd import _lib as L
    rs = np.random.RandomState(8)
    for cs, lo, hi, wave in (([65, 40], 4, 20, True), ([9, 7, 30], 2, 6, True), ([8, 9, 30], 2, 6, True),
                             ([64, 40], 4, 20, False), ([8, 8, 30], 2, 6, False)):
        D, B, n = len(cs), 6, 6
        blocks = _blocks(rs, B, n, D, lo, hi, 1, 4)
        want = _oracle(cs, "C+P+S-mcs-soft", blocks)
        assert want["nerr"] == 0
        L.variant_hits_reset(DEV)
        rc, pos, st, rew, s64 = _pack_blocks(L, cs, n, "C+P+S-mcs-soft", blocks)
        assert rc == L.TAP_OK, (cs, rc)
        assert np.array_equal(pos, want["positions"]) and np.array_equal(_bits(s64), _bits(want["ratio"])), cs
        hits = _hits(L, (_wave_kind(L, D),) + _lane_kinds(L))
        kind = _wave_kind(L, D) if wave else (L.TAP_HIT_EPISODE_MACS2 if D == 2 else L.TAP_HIT_EPISODE_MACS3)
        assert list(hits.values()) == [1] and next(iter(hits))[0] == kind, (cs, hits)


def test_large_batch_takes_the_register_tight_build(T):
    """k_macs3d_wave_episode exists in two register builds (macs3_big.hip); the launcher takes the tight one when a CU
    would hold more waves than the loose one's registers allow: 10 x 10 at B = 4 096 (16 waves per CU on 256 CUs, a
    5 KiB tile).  The launch record says which build ran (mode 1 = tight); every container against the stepped path,
    error words included, and the first 64 against the oracle.  The small batches of the other tests run the loose
    build (mode 0, asserted there)."""
    from tap_net_amd import _lib as L, pack
    cs, n, B, reward = [10, 10, 50], 8, 4096, "C+P+S-mcs-soft"
    blocks = _blocks(np.random.RandomState(77), B, n, 3, 2, 6)
    static, R = _static_of(blocks)
    g = torch.Generator().manual_seed(9)
    tour = torch.stack([torch.randperm(n if b % 2 == 0 else n * R, generator=g)[:n] for b in range(B)]).to(DEV)
    L.variant_hits_reset(DEV)
    rc, ratio, scores, err = _episode_scores(L, cs, n, reward, static, tour)
    assert rc == L.TAP_OK, rc
    hits = _hits(L, (L.TAP_HIT_EPISODE_MACS3_WAVE,) + _lane_kinds(L))
    assert hits == {(L.TAP_HIT_EPISODE_MACS3_WAVE, 3, 64, 0, 1, 4, 0): 1}, hits
    r_s, s_s = pack._stepped_scores(static, tour, cs, n, reward, "MACS", None, check=False)
    assert _same_f64(ratio, r_s.cpu().numpy())
    assert np.array_equal(scores, s_s.cpu().numpy())
    assert np.array_equal(err, _stepped_errors(T, cs, n, reward, static, tour))
    assert not err.any() and int((scores[:, 4] > 5).sum()) > 0                   # no error; a map above 5, the tallest block, means stacking
    w = _oracle(cs, reward, _gather(static[:64], tour[:64], 3))
    assert w["nerr"] == 0
    assert np.array_equal(_bits(ratio[:64]), _bits(w["ratio"])) and np.array_equal(scores[:64], w["scores"])
