"""The fused 2D step of the reference's own window (n = 10: 30 rows, nR = 20) in its common form -- on the bit shadow,
every input given, whole workgroups: k_transition<2, G, 1, 4, 77> -- runs update_mask on one mask wave per workgroup
(tap_masks.h: mask_wave_bits) while its stream waves keep update_dynamic.  Three consecutive tap_transition_bits steps
for G = 8 / 16 / 32 against the two-launch path (tap_mask_step_bits + tap_env_step_gather), which defines the behaviour,
and against the CPU oracle; every comparison is on bit patterns.  Also: old-mask values other than 0 / 1 pass through, a
pick outside [0, nR) clears nothing and removes no column, and the three mask buffers need no more than float alignment."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
N, ROWS, R, NR, STEPS = 10, 30, 2, 20, 3
SV_TRANSITION = 0                    # tap_stream_variant.h: TAP_SV_TRANSITION
MODE_MASK_WAVE = 1 | 4 | 8 | 64      # shadow | run-of-rows | shape 5 | FULL: the instantiation with the mask wave
MODE_RAGGED = 1 | 4 | 8              # the same without FULL (B no multiple of the workgroup's envs): unchanged


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


_instances = {}


def _instance(B):
    """(static, dynamic, tape) of one batch size, made once and shared (never modified)."""
    if B not in _instances:
        from tap_net_amd import synth
        static, dynamic = synth.rand_instances(B, N, 2, seed=100 + B)
        _instances[B] = (static, dynamic, synth.random_feasible_tape(static, dynamic, N, seed=7 + B))
    return _instances[B]


def _bits_of(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _same(got, want, what):
    g, w = _bits_of(got), _bits_of(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert len(bad) == 0, "%s: %d mismatches, first at %s" % (what, len(bad), bad[0].tolist())


def _window(B, offset):
    """A (B, nR) fp32 tensor that starts `offset` bytes into its allocation."""
    buf = torch.full((B * NR + 16,), 7.5, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 64 == 0 and offset % 4 == 0
    w = buf[offset // 4: offset // 4 + B * NR].view(B, NR)
    assert w.data_ptr() % 16 == offset % 16
    return buf, w


def _expand(bits, B):
    r = torch.arange(ROWS, device=bits.device)
    return ((bits.view(B, 1, NR) >> r.view(1, -1, 1)) & 1).to(torch.float32)


def _run(T, cs, B, mask0=None, bad_picks=False, offset=0, oracle=True, mode=MODE_MASK_WAVE):
    """STEPS steps through tap_transition_bits and through the two launches, compared after every step."""
    from tap_net_amd import pack
    L, lib = T._lib, T._lib.lib()
    static, dynamic, tape = _instance(B)
    st, dy = static.to(DEV), dynamic.to(DEV)
    ctx, stream = L.ctx(DEV), L.stream_of(torch.device(DEV))
    bits0 = pack.dynamic_bits(dy)[0]
    assert bits0.data_ptr() % 16 == 0
    envs = [T.BatchedContainer(B, list(cs), N, "C+P+S-lb-soft", "diff", device=DEV) for _ in range(2)]
    for e in envs:
        e.reset()
    feats = [torch.empty(envs[0]._feature_shape(), device=DEV) for _ in range(2)]
    # per path: two phases of shadow / tensor / masks; the masks may sit `offset` bytes into their allocations
    keep = []
    state = []
    for _ in range(2):
        ph = []
        for _w in range(2):
            mb, m = _window(B, offset)
            cb, c = _window(B, offset)
            keep += [mb, cb]
            ph.append(dict(bits=torch.empty_like(bits0), dyn=torch.empty(B, ROWS, NR, device=DEV), mask=m, cur=c, mbuf=mb, cbuf=cb))
        state.append(ph)
    ib, m_in = _window(B, offset)
    if mask0 is None:
        m_in.fill_(1.0)
    else:
        m_in.copy_(mask0.to(DEV))
    in_bits = _bits_of(m_in).copy()
    stn, tp = static.numpy(), tape.numpy().copy()
    if bad_picks:                      # second step: a quarter of the envs pick -1, another quarter nR
        tp[0:B:4, 1] = -1
        tp[1:B:4, 1] = NR
    dyn_ref, mask_ref = dynamic.numpy().copy(), np.ones((B, NR), np.float32)
    if oracle:
        blocks = np.stack([stn[np.arange(B), 1:, tp[:, t]] for t in range(STEPS)], axis=1).astype(np.int32)
        ref = O.run_episodes(O.make_desc(list(cs), N, "C+P+S-lb-soft", "diff"), blocks)
    L.variant_hits_reset(DEV)
    for t in range(STEPS):
        ptr = torch.from_numpy(tp[:, t].copy()).to(DEV)
        w, r = t & 1, (t & 1) ^ 1
        src = [(bits0, m_in) if t == 0 else (state[k][r]["bits"], state[k][r]["mask"]) for k in range(2)]
        f, s = state[0][w], state[1][w]
        L.check(lib.tap_transition_bits(ctx, C.byref(envs[0].desc), L.ptr(envs[0]._state), N, R, ROWS, 3, L.ptr(src[0][0]),
                                        L.ptr(st), st.shape[1], L.ptr(ptr), L.ptr(src[0][1]), L.ptr(f["bits"]), L.ptr(f["dyn"]),
                                        L.ptr(f["cur"]), L.ptr(f["mask"]), L.ptr(feats[0]), None,
                                        L.TAP_T_FRESH if t == 0 else 0, stream), ctx)
        L.check(lib.tap_mask_step_bits(ctx, B, N, R, ROWS, 3, L.ptr(src[1][0]), L.ptr(st), st.shape[1], L.ptr(ptr),
                                       L.ptr(src[1][1]), L.ptr(s["bits"]), L.ptr(s["dyn"]), L.ptr(s["cur"]), L.ptr(s["mask"]),
                                       stream), ctx)
        L.check(lib.tap_env_step_gather(ctx, C.byref(envs[1].desc), L.ptr(envs[1]._state), L.ptr(st), st.shape[1], NR,
                                        L.ptr(ptr), None, L.ptr(feats[1]), stream), ctx)
        torch.cuda.synchronize()
        where = "%s B %d step %d" % ("x".join(map(str, cs)), B, t)
        for what in ("dyn", "bits", "mask", "cur"):
            _same(f[what], s[what], what + " against the two launches, " + where)
        # nothing outside the windows was written
        for what in ("mbuf", "cbuf"):
            lo, hi = offset // 4, offset // 4 + B * NR
            assert bool((f[what][:lo] == 7.5).all()) and bool((f[what][hi:] == 7.5).all()), what + " guard, " + where
        if not bad_picks:
            _same(feats[0], feats[1], "feature, " + where)
            for what in ("positions", "heightmap", "counters", "stable"):
                a, b = getattr(envs[0], what), getattr(envs[1], what)
                assert torch.equal(a, b), what + ", " + where
        if oracle:
            p = tp[:, t]
            dyn_ref = O.update_dynamic(dyn_ref, stn, p, N, 3)
            cur_ref, mask_ref = O.update_mask(mask_ref, dyn_ref, p, N, R)
            for what, got, want in (("dyn", f["dyn"], dyn_ref), ("shadow", _expand(f["bits"], B), dyn_ref),
                                    ("mask", f["mask"], mask_ref), ("cur", f["cur"], cur_ref)):
                assert np.array_equal(_bits_of(got), np.ascontiguousarray(want).view(np.int32)), what + " against the oracle, " + where
            assert np.array_equal(feats[0].reshape(B, -1).to(torch.int64).cpu().numpy(), ref["features"][:, t]), "feature against the oracle, " + where
    assert np.array_equal(_bits_of(m_in), in_bits), "mask_in was written"
    if oracle:
        want = ref["positions"].reshape(B, -1)
        assert np.array_equal(envs[0].positions.cpu().numpy().reshape(B, -1)[:, :want.shape[1]], want)
    # the launch record: every fused step ran the instantiation this file is about
    got = {k for k in L.variant_keys(DEV) if k[0] == SV_TRANSITION}
    G = 8 if cs[0] <= 8 else 16 if cs[0] <= 16 else 32
    assert got == {(SV_TRANSITION, 2, G, 1, mode, 0, 1)}, got
    return state[0]


@pytest.mark.parametrize("B", [8, 16, 40])
@pytest.mark.parametrize("cs", [(5, 50), (12, 40), (30, 60)], ids=lambda c: "%dx%d" % c)
def test_three_steps_against_two_launches_and_oracle(T, cs, B):
    _run(T, cs, B)


def test_ragged_batch_keeps_the_stream_wave_tail(T):
    """B = 13 is no multiple of the workgroup's 8 envs: the instantiation without FULL, which has no mask wave."""
    _run(T, (5, 50), 13, mode=MODE_RAGGED)


def test_old_mask_values_pass_through(T):
    """mask_in holding 0, 1, 0.5 and -0.0: kept bit for bit where the pick does not remove the column (the two-launch
    path defines the behaviour; the oracle's update_mask is for 0 / 1 masks)."""
    B = 16
    vals = torch.tensor([0.0, 1.0, 0.5, -0.0])
    m0 = vals[torch.from_numpy(np.random.RandomState(3).randint(0, 4, size=(B, NR)))]
    out = _run(T, (5, 50), B, mask0=m0, oracle=False)
    last = _bits_of(out[(STEPS - 1) & 1]["mask"])
    kept = _bits_of(m0)
    # -0.0 and 0.5 survive in the columns no pick removed; removed columns are +0.0
    assert ((last == kept) | (last == 0)).all()
    assert (last == np.float32(0.5).view(np.int32)).any() and (last == np.float32(-0.0).view(np.int32)).any()


def test_out_of_range_picks_agree_with_two_launches(T):
    """-1 in a quarter of the envs' picks at the second step, nR in another quarter: the precedence outputs of both
    paths agree (nothing cleared, no column removed); nothing is asserted about the placement of such a pick."""
    _run(T, (5, 50), 16, bad_picks=True, oracle=False)
    _run(T, (30, 60), 8, bad_picks=True, oracle=False)


@pytest.mark.parametrize("offset", [4, 16], ids=["4-bytes", "16-bytes"])
def test_mask_buffers_at_an_offset(T, offset):
    """mask_in, mask_out and current_out each start `offset` bytes into their allocation: only dyn_* and bits_* are
    promised 16-byte aligned."""
    _run(T, (5, 50), 16, offset=offset)
    _run(T, (12, 40), 8, offset=offset)
