"""The fused 2D step whose stream waves take their inputs with two vector loads and hand the shadow words round through
the wave's LDS tile (tap_masks.h: stream_wave_bits_r4, NOMASK path; k_transition<2, G, 1, 4, 77>, G = 8 / 16 / 32).

Through the C ABI: ten steps of tap_transition_bits on the 10-node 2D window (n = 10, R = 2, rows = 30, nR = 20,
update_rows = 3) from a tap_dyn_bits shadow of a random 0/1 tensor.  After EVERY step the outputs equal, bit for bit, those
of the two-launch path (tap_mask_step_bits + tap_env_step_gather) and oracle_lib.update_dynamic / update_mask; every
output buffer is poisoned (NaN / all-ones) before the step, so an element the step does not write cannot compare equal.
Each case asserts on the launch record that the mode-77 instantiation of its lane group ran.

The picks put column 0, 9, 10 and 19 into slab 0 and into slab 1 of one stream wave (different picks in the two slabs --
the pick is read at lane p for slab 0 and at lane 20 + p for slab 1), column 19 into the last env of the last workgroup,
and ptr = -1 / ptr = nR (clear nothing, remove no column) into both slabs of a wave."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
N, R, ROWS, NR, UR, STEPS = 10, 2, 30, 20, 3, 10
MODE_77 = 77                                  # shadow | run-of-rows | shape 5 | FULL (tap_stream_variant.h)
WIDTH_G = ((5, 8), (12, 16), (20, 32))        # container width -> lane group (tap_common.h: tap_group_size, cells = W in 2D)
BATCHES = (8, 24, 1032)                       # one workgroup, three, and 129: more than one per XCD, an odd count


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


def _eq(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = want.cpu().numpy() if torch.is_tensor(want) else want
    assert got.shape == want.shape, "%s: shape %s != %s" % (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %d mismatches, first at %s" % (what, int((got != want).sum()),
                                                                           np.argwhere(got != want)[0].tolist())


def _pack(dyn):
    """(B, rows, nR) 0/1 floats -> (B, nR) int64 column words, bit r = dyn[b, r, j] != 0"""
    w = np.zeros((dyn.shape[0], dyn.shape[2]), np.int64)
    for r in range(dyn.shape[1]):
        w |= (dyn[:, r, :] != 0).astype(np.int64) << r
    return w


def _picks(B, seed):
    """(B, STEPS) int64: random columns, then the ones that stress the lane mapping; bad[b, t]: ptr outside [0, nR)"""
    rng = np.random.RandomState(seed)
    p = rng.randint(0, NR, size=(B, STEPS)).astype(np.int64)
    p[0, :4] = (0, 9, 10, 19)                 # slab 0 of workgroup 0's first stream wave
    p[1, :4] = (19, 10, 0, 9)                 # slab 1 of the same wave: never the same pick as slab 0
    p[B - 2, :4] = (19, 0, 9, 10)             # the last wave of the last workgroup
    p[B - 1, :4] = (0, 19, 10, 9)
    p[B - 1, 5] = 19
    p[2, 4], p[3, 4] = -1, NR                 # both slabs of one wave select nothing
    p[4, 6], p[5, 7] = NR, -1                 # one slab of a wave selects nothing, the other a column
    return p, (p < 0) | (p >= NR)


@pytest.fixture(scope="module")
def inputs():
    """static (sizes and block ids of synthetic instances), a random 0/1 dynamic and the picks, per batch size"""
    from tap_net_amd import synth
    out = {}
    for B in BATCHES:
        static, _ = synth.rand_instances(B, N, 2, seed=100 + B)
        dyn = (np.random.RandomState(B).random_sample((B, ROWS, NR)) < 0.4).astype(np.float32)
        out[B] = (static.contiguous(), torch.from_numpy(dyn)) + _picks(B, seed=7 + B)
    return out


def _episode(T, W, G, B, inputs, high_seed=None, steps=STEPS):
    L, lib = T._lib, T._lib.lib()
    static, dynamic, picks, bad = inputs[B]
    st, dy = static.to(DEV), dynamic.to(DEV)
    ctx, stream = L.ctx(DEV), L.stream_of(torch.device(DEV))
    fused = T.BatchedContainer(B, [W, 50], N, "C+P+S-lb-soft", "diff", device=DEV)
    two = T.BatchedContainer(B, [W, 50], N, "C+P+S-lb-soft", "diff", device=DEV)
    bits = torch.empty(B, NR, dtype=torch.int64, device=DEV)
    L.check(lib.tap_dyn_bits(ctx, B, NR, ROWS, L.ptr(dy), L.ptr(bits), None, stream), ctx)
    _eq(bits, _pack(dynamic.numpy()), "tap_dyn_bits")
    high = np.zeros((B, NR), np.int64)
    if high_seed is not None:                 # random bits 30 .. 63 ride in the words; the step must carry them along
        high = np.random.RandomState(high_seed).randint(0, 1 << 34, size=(B, NR), dtype=np.int64) << ROWS
        bits |= torch.from_numpy(high).to(DEV)
    mask = torch.ones(B, NR, device=DEV)
    stn, dyn_ref, mask_ref = static.numpy(), dynamic.numpy().copy(), np.ones((B, NR), np.float32)
    nan = float("nan")
    L.variant_hits_reset(DEV)
    for t in range(steps):
        p_np, bad_t = picks[:, t], bad[:, t]
        ptr = torch.from_numpy(p_np.copy()).to(DEV)
        f = dict(bits=torch.full((B, NR), -1, dtype=torch.int64, device=DEV), dyn=torch.full((B, ROWS, NR), nan, device=DEV),
                 cur=torch.full((B, NR), nan, device=DEV), mask=torch.full((B, NR), nan, device=DEV),
                 feat=torch.full(fused._feature_shape(), nan, device=DEV))
        g = {k: v.clone() for k, v in f.items()}
        L.check(lib.tap_transition_bits(ctx, C.byref(fused.desc), L.ptr(fused._state), N, R, ROWS, UR, L.ptr(bits), L.ptr(st),
                                        st.shape[1], L.ptr(ptr), L.ptr(mask), L.ptr(f["bits"]), L.ptr(f["dyn"]), L.ptr(f["cur"]),
                                        L.ptr(f["mask"]), L.ptr(f["feat"]), None, 0, stream), ctx)
        L.check(lib.tap_mask_step_bits(ctx, B, N, R, ROWS, UR, L.ptr(bits), L.ptr(st), st.shape[1], L.ptr(ptr), L.ptr(mask),
                                       L.ptr(g["bits"]), L.ptr(g["dyn"]), L.ptr(g["cur"]), L.ptr(g["mask"]), stream), ctx)
        two.add_new_blocks_gather(st, ptr, out=g["feat"])
        torch.cuda.synchronize()
        where = "W %d B %d step %d" % (W, B, t)
        # the oracle raises for an index outside [0, nR), like the reference's gather: those envs keep what they had
        prev_dyn, prev_mask = dyn_ref, mask_ref
        safe = np.where(bad_t, 0, p_np)
        dyn_ref = O.update_dynamic(prev_dyn, stn, safe, N, UR)
        dyn_ref[bad_t] = prev_dyn[bad_t]
        cur_ref, mask_ref = O.update_mask(prev_mask, dyn_ref, safe, N, R)
        mask_ref[bad_t] = prev_mask[bad_t]
        ok = ~bad_t
        for k in ("dyn", "cur", "mask", "feat"):
            assert not torch.isnan(f[k]).any(), "%s: %s keeps poisoned elements" % (where, k)
            _eq(f[k], g[k], "%s against the two-launch path, %s" % (k, where))
        _eq(f["dyn"], dyn_ref, "dyn_out against the oracle, " + where)
        _eq(f["mask"], mask_ref, "mask_out against the oracle, " + where)
        _eq(f["cur"][torch.from_numpy(ok).to(DEV)], cur_ref[ok], "current_out against the oracle, " + where)
        # all 64 bits of a word: the rows of the new tensor below, whatever the input word held above
        _eq(f["bits"], _pack(dyn_ref) | high, "bits_out against the oracle, " + where)
        if high_seed is None:
            _eq(f["bits"], g["bits"], "bits_out against the two-launch path, " + where)
        _eq(fused.heightmap, two.heightmap, "heightmap, " + where)
        _eq(fused.positions, two.positions, "positions, " + where)
        bits, mask = f["bits"], f["mask"]
    hits = L.variant_hits(DEV)
    key = (0, 2, G, 1, MODE_77, 0, 1)
    assert hits.get(key) == steps, "k_transition<2, %d, 1, 4, 77> (write-through) launched %r times, record: %s" % (
        G, hits.get(key), sorted(hits))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("W,G", WIDTH_G, ids=["G%d" % g for _, g in WIDTH_G])
def test_ten_steps_equal_the_two_launch_path_and_the_oracle(T, inputs, W, G, B):
    _episode(T, W, G, B, inputs)


def test_bits_30_to_63_of_a_shadow_word_pass_through(T, inputs):
    """A shadow whose words carry random bits 30 .. 63: bits_out = bits_in & ~clear in all 64 bits, and every other output
    is what the clean shadow gives (the expansion and the masks read rows 0 .. 29 only)."""
    _episode(T, 5, 8, 24, inputs, high_seed=3, steps=4)
