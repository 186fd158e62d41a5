"""The first step of an episode on the reference's own windows (n = 10: 30 rows, nR = 20 in 2D / 60 in 3D) --
k_transition<2, G, 1, 4, 14> (run-of-rows, write-through), <2, G, 1, 4, 10> (slab by slab, nontemporal) and
<3, G, 1, 8, 18> -- builds the bit shadow from the fp32 tensor inside the launch and writes update_dynamic's result as
fp32 (tap_masks.h: the BUILD branch of stream_wave_bits_r4).  One tap_transition_first and two tap_transition_bits steps
against the two-launch path (tap_mask_step_first + tap_env_step_gather, then tap_mask_step_bits), which defines the
behaviour, and against the CPU oracle; every comparison is on bit patterns.  Also: tensors that are not 0 / 1 (the stored
value is +0.0 in a cleared row, else 1.0 where the element is non-zero, else +0.0; the counter of elements that are
neither 0 nor 1 includes the cleared rows), picks outside [0, nR), old-mask values other than 0 / 1, the step object's
first step without a mask, outputs at a 16-byte offset inside guard-filled allocations, and launches beyond the
write-through limit."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
N, ROWS, STEPS = 10, 30, 3
SV_TRANSITION = 0                    # tap_stream_variant.h: TAP_SV_TRANSITION
MODE_2D, MODE_2D_NT, MODE_3D = 2 | 4 | 8, 2 | 8, 2 | 16
GUARD = 7.5


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


_instances = {}


def _instance(D, B):
    """(static, dynamic, tape) of one dimension and batch size, made once and shared (never modified)."""
    if (D, B) not in _instances:
        from tap_net_amd import synth
        static, dynamic = synth.rand_instances(B, N, D, seed=300 + 7 * D + B)
        _instances[(D, B)] = (static, dynamic, synth.random_feasible_tape(static, dynamic, N, seed=11 + B))
    return _instances[(D, B)]


def _tiled(D, B, base=40):
    """A batch of B envs made of the shared `base`-env instance, repeated."""
    static, dynamic, tape = _instance(D, base)
    rep = (B + base - 1) // base
    return tuple(t.repeat((rep,) + (1,) * (t.dim() - 1))[:B].contiguous() for t in (static, dynamic, tape))


def _bits_of(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64).cpu().numpy()


def _same(got, want, what):
    g, w = _bits_of(got), _bits_of(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert len(bad) == 0, "%s: %d mismatches, first at %s" % (what, len(bad), bad[0].tolist())


def _group(cs):
    cells = int(np.prod(cs[:-1]))
    return 8 if cells <= 8 else 16 if cells <= 16 else 32 if cells <= 32 else 64


def _guarded(shape, dtype, offset):
    """A tensor of `shape` that starts `offset` bytes into a guard-filled allocation -> (allocation, view, lo, hi)."""
    numel, esz = int(np.prod(shape)), torch.empty(0, dtype=dtype).element_size()
    pad = 64 // esz
    buf = torch.full((numel + 2 * pad,), GUARD if dtype.is_floating_point else 0x5a5a5a5a, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 64 == 0 and offset % esz == 0
    lo = offset // esz
    view = buf[lo:lo + numel].view(shape)
    assert view.data_ptr() % 16 == offset % 16
    return buf, view, lo, lo + numel


def _guard_ok(buf, lo, hi):
    fill = buf.new_tensor(GUARD if buf.dtype.is_floating_point else 0x5a5a5a5a)
    return bool((buf[:lo] == fill).all()) and bool((buf[hi:] == fill).all())


def _run(T, cs, B, mode, inst=None, dyn0=None, mask0=None, bad_picks=False, offset=0, oracle=True, wt=1, steps=STEPS):
    """`steps` steps, the first through tap_transition_first, on the fused path and through the two launches, compared
    after every step.  -> (phases of the fused path, its non-binary count)."""
    L, lib = T._lib, T._lib.lib()
    D = len(cs)
    R = 2 if D == 2 else 6
    NR = N * R
    static, dynamic, tape = inst if inst is not None else _instance(D, B)
    if dyn0 is not None:
        dynamic = dyn0
    st, dy = static.to(DEV), dynamic.to(DEV)
    dy_bits = _bits_of(dy).copy()
    ctx, stream = L.ctx(DEV), L.stream_of(torch.device(DEV))
    envs = [T.BatchedContainer(B, list(cs), N, "C+P+S-lb-soft", "diff", device=DEV) for _ in range(2)]
    for e in envs:
        e.reset()
    feats = [torch.empty(envs[0]._feature_shape(), device=DEV) for _ in range(2)]
    state = []
    for _ in range(2):
        ph = []
        for _w in range(2):
            bb, bits, blo, bhi = _guarded((B, NR), torch.int64, offset)
            db, dyn, dlo, dhi = _guarded((B, ROWS, NR), torch.float32, offset)
            ph.append(dict(bits=bits, dyn=dyn, mask=torch.empty(B, NR, device=DEV), cur=torch.empty(B, NR, device=DEV),
                           guards=((bb, blo, bhi, "bits_out"), (db, dlo, dhi, "dyn_out"))))
        state.append(ph)
    m_in = torch.ones(B, NR, device=DEV) if mask0 is None else mask0.to(DEV)
    in_bits = _bits_of(m_in).copy()
    counts = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2)]
    stn, tp = static.numpy(), tape.numpy().copy()
    if bad_picks:                      # first step: a quarter of the envs pick -1, another quarter nR
        tp[0:B:4, 0] = -1
        tp[1:B:4, 0] = NR
    dyn_ref, mask_ref = dynamic.numpy().copy(), np.ones((B, NR), np.float32)
    if oracle:
        blocks = np.stack([stn[np.arange(B), 1:, tp[:, t]] for t in range(steps)], axis=1).astype(np.int32)
        ref = O.run_episodes(O.make_desc(list(cs), N, "C+P+S-lb-soft", "diff"), blocks)
    L.variant_hits_reset(DEV)
    for t in range(steps):
        ptr = torch.from_numpy(tp[:, t].copy()).to(DEV)
        w, r = t & 1, (t & 1) ^ 1
        f, s = state[0][w], state[1][w]
        if t == 0:
            L.check(lib.tap_transition_first(ctx, C.byref(envs[0].desc), L.ptr(envs[0]._state), N, R, ROWS, 3, L.ptr(dy), L.ptr(st),
                                             st.shape[1], L.ptr(ptr), L.ptr(m_in), L.ptr(f["bits"]), L.ptr(f["dyn"]), L.ptr(f["cur"]),
                                             L.ptr(f["mask"]), L.ptr(feats[0]), None, L.ptr(counts[0]), L.TAP_T_FRESH, stream), ctx)
            L.check(lib.tap_mask_step_first(ctx, B, N, R, ROWS, 3, L.ptr(dy), L.ptr(st), st.shape[1], L.ptr(ptr), L.ptr(m_in),
                                            L.ptr(s["bits"]), L.ptr(s["dyn"]), L.ptr(s["cur"]), L.ptr(s["mask"]), L.ptr(counts[1]),
                                            stream), ctx)
        else:
            src = [(state[k][r]["bits"], state[k][r]["mask"]) for k in range(2)]
            L.check(lib.tap_transition_bits(ctx, C.byref(envs[0].desc), L.ptr(envs[0]._state), N, R, ROWS, 3, L.ptr(src[0][0]),
                                            L.ptr(st), st.shape[1], L.ptr(ptr), L.ptr(src[0][1]), L.ptr(f["bits"]), L.ptr(f["dyn"]),
                                            L.ptr(f["cur"]), L.ptr(f["mask"]), L.ptr(feats[0]), None, 0, stream), ctx)
            L.check(lib.tap_mask_step_bits(ctx, B, N, R, ROWS, 3, L.ptr(src[1][0]), L.ptr(st), st.shape[1], L.ptr(ptr),
                                           L.ptr(src[1][1]), L.ptr(s["bits"]), L.ptr(s["dyn"]), L.ptr(s["cur"]), L.ptr(s["mask"]),
                                           stream), ctx)
        L.check(lib.tap_env_step_gather(ctx, C.byref(envs[1].desc), L.ptr(envs[1]._state), L.ptr(st), st.shape[1], NR,
                                        L.ptr(ptr), None, L.ptr(feats[1]), stream), ctx)
        torch.cuda.synchronize()
        where = "%s B %d step %d" % ("x".join(map(str, cs)), B, t)
        for what in ("dyn", "bits", "mask", "cur"):
            _same(f[what], s[what], what + " against the two launches, " + where)
        for buf, lo, hi, what in f["guards"]:
            assert _guard_ok(buf, lo, hi), what + " guard, " + where
        if t == 0:
            assert int(counts[0].item()) == int(counts[1].item()), "non-binary count, " + where
            assert np.array_equal(_bits_of(dy), dy_bits), "dyn_in was written, " + where
        if not bad_picks:
            _same(feats[0], feats[1], "feature, " + where)
            for what in ("positions", "heightmap", "counters", "stable"):
                a, b = getattr(envs[0], what), getattr(envs[1], what)
                assert torch.equal(a, b), what + ", " + where
        if oracle:
            p = tp[:, t]
            dyn_ref = O.update_dynamic(dyn_ref, stn, p, N, 3)
            cur_ref, mask_ref = O.update_mask(mask_ref, dyn_ref, p, N, R)
            r_ = torch.arange(ROWS, device=DEV)
            shadow = ((f["bits"].view(B, 1, NR) >> r_.view(1, -1, 1)) & 1).to(torch.float32)
            for what, got, want in (("dyn", f["dyn"], dyn_ref), ("shadow", shadow, dyn_ref),
                                    ("mask", f["mask"], mask_ref), ("cur", f["cur"], cur_ref)):
                assert np.array_equal(_bits_of(got), np.ascontiguousarray(want).view(np.int32)), what + " against the oracle, " + where
            assert np.array_equal(feats[0].reshape(B, -1).to(torch.int64).cpu().numpy(), ref["features"][:, t]), "feature against the oracle, " + where
    assert np.array_equal(_bits_of(m_in), in_bits), "mask_in was written"
    # the launch record: the first step ran the instantiation this file is about
    got = {k for k in L.variant_keys(DEV) if k[0] == SV_TRANSITION and (k[4] & 3) == 2}
    assert got == {(SV_TRANSITION, D, _group(cs), 1, mode, 0, wt)}, got
    return state[0], int(counts[0].item())


@pytest.mark.parametrize("B", [8, 13, 40])
@pytest.mark.parametrize("cs", [(5, 50), (12, 40), (30, 60)], ids=lambda c: "x".join(map(str, c)))
def test_2d_first_step_against_two_launches_and_oracle(T, cs, B):
    """G = 8 / 16 / 32, two slabs per stream wave.  B = 8: one workgroup; 13: a wave with an idle second slab and idle
    waves; 40: five workgroups."""
    _run(T, cs, B, MODE_2D)


@pytest.mark.parametrize("cs,B", [((5, 5, 50), 4), ((5, 5, 50), 5), ((5, 5, 50), 24), ((8, 8, 50), 4), ((8, 8, 50), 5),
                                  ((8, 8, 50), 24), ((2, 2, 50), 5)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_3d_first_step_against_two_launches_and_oracle(T, cs, B):
    """G = 32 (eight envs per workgroup), G = 64 (four) and G = 8; one slab per stream wave."""
    _run(T, cs, B, MODE_3D)


def _scatter(dynamic, static, tape, seed):
    """0.5, 2.0, -0.0, -1.0 and NaN over a 0/1 tensor: at random places and, per env, in the rows the first pick clears.
    -> (tensor, number of elements that are neither 0 nor 1)."""
    rng = np.random.RandomState(seed)
    d = dynamic.numpy().copy()
    B, rows, nR = d.shape
    vals = np.array([0.5, 2.0, -0.0, -1.0, np.nan], np.float32)
    idx = rng.choice(d.size, size=max(5, d.size // 25), replace=False)
    d.reshape(-1)[idx] = vals[np.arange(len(idx)) % len(vals)]
    real = static.numpy()[np.arange(B), 0, tape.numpy()[:, 0]].astype(np.int64)
    for b in range(B):
        for i in range(3):
            if real[b] + N * i < rows:
                d[b, real[b] + N * i, rng.randint(nR)] = vals[(b + i) % len(vals)]
    bad = int(((d != 0) & (d != 1)).sum())
    assert bad > 0 and np.signbit(d[d == 0]).any()
    return torch.from_numpy(d), bad


@pytest.mark.parametrize("cs,B,mode", [((5, 50), 13, MODE_2D), ((30, 60), 16, MODE_2D), ((5, 5, 50), 5, MODE_3D), ((8, 8, 50), 8, MODE_3D)],
                         ids=["5x50", "30x60", "5x5x50", "8x8x50"])
def test_tensor_that_is_not_binary(T, cs, B, mode):
    """The two-launch path defines the result (the oracle is for 0 / 1 tensors): dyn_out, the shadow and both masks bit
    for bit, the count of elements that are neither 0 nor 1 (cleared rows included), dyn_in untouched."""
    static, dynamic, tape = _instance(len(cs), B)
    d0, bad = _scatter(dynamic, static, tape, seed=5 + B)
    out, count = _run(T, cs, B, mode, dyn0=d0, oracle=False)
    assert count == bad
    got = _bits_of(out[0]["dyn"])
    assert set(np.unique(got).tolist()) <= {0, int(np.float32(1.0).view(np.int32))}   # +0.0 or 1.0, nothing else


def test_out_of_range_first_picks(T):
    """-1 in a quarter of the envs' first picks, nR in another quarter: nothing cleared, no column removed; nothing is
    asserted about the placement of such a pick."""
    _run(T, (5, 50), 16, MODE_2D, bad_picks=True, oracle=False)
    _run(T, (5, 50), 13, MODE_2D, bad_picks=True, oracle=False)
    _run(T, (5, 5, 50), 8, MODE_3D, bad_picks=True, oracle=False)


def test_old_mask_values_pass_through(T):
    """mask_in holding 0, 1, 0.5 and -0.0: kept bit for bit where the pick does not remove the column."""
    for cs, B, mode in (((5, 50), 16, MODE_2D), ((5, 5, 50), 8, MODE_3D)):
        nR = N * (2 if len(cs) == 2 else 6)
        vals = torch.tensor([0.0, 1.0, 0.5, -0.0])
        m0 = vals[torch.from_numpy(np.random.RandomState(3).randint(0, 4, size=(B, nR)))]
        out, _ = _run(T, cs, B, mode, mask0=m0, oracle=False)
        first, kept = _bits_of(out[0]["mask"]), _bits_of(m0)
        assert ((first == kept) | (first == 0)).all()
        assert (first == np.float32(0.5).view(np.int32)).any() and (first == np.float32(-0.0).view(np.int32)).any()


@pytest.mark.parametrize("cs,B", [((5, 50), 13), ((5, 5, 50), 5)], ids=["5x50", "5x5x50"])
@pytest.mark.parametrize("initial_mask", [False, True], ids=["no-mask_in", "initial-mask"])
def test_step_object_first_step(T, cs, B, initial_mask):
    """pack.EpisodeStepper.begin(initial_mask=False): step 0 is the first-step kernel WITHOUT mask_in (ones);
    initial_mask=True: begin's own launch builds shadow and masks.  Both against the two launches with a mask of ones."""
    from tap_net_amd import pack
    L, lib = T._lib, T._lib.lib()
    D = len(cs)
    R = 2 if D == 2 else 6
    NR = N * R
    static, dynamic, tape = _instance(D, B)
    st, dy, tp = static.to(DEV), dynamic.to(DEV), tape.to(DEV)
    ctx, stream = L.ctx(DEV), L.stream_of(torch.device(DEV))
    env = T.BatchedContainer(B, list(cs), N, "C+P+S-lb-soft", "diff", device=DEV)
    sp = pack.EpisodeStepper(st, dy, env, steps=STEPS)
    sp.begin(st, dy, initial_mask=initial_mask)
    ph = [dict(bits=torch.empty(B, NR, dtype=torch.int64, device=DEV), dyn=torch.empty(B, ROWS, NR, device=DEV),
               mask=torch.empty(B, NR, device=DEV), cur=torch.empty(B, NR, device=DEV)) for _ in range(2)]
    ones, cnt = torch.ones(B, NR, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    for t in range(STEPS):
        ptr = tp[:, t].contiguous()
        w, r = t & 1, (t & 1) ^ 1
        s = ph[w]
        if t == 0:
            L.check(lib.tap_mask_step_first(ctx, B, N, R, ROWS, 3, L.ptr(dy), L.ptr(st), st.shape[1], L.ptr(ptr), L.ptr(ones),
                                            L.ptr(s["bits"]), L.ptr(s["dyn"]), L.ptr(s["cur"]), L.ptr(s["mask"]), L.ptr(cnt), stream), ctx)
        else:
            L.check(lib.tap_mask_step_bits(ctx, B, N, R, ROWS, 3, L.ptr(ph[r]["bits"]), L.ptr(st), st.shape[1], L.ptr(ptr),
                                           L.ptr(ph[r]["mask"]), L.ptr(s["bits"]), L.ptr(s["dyn"]), L.ptr(s["cur"]), L.ptr(s["mask"]),
                                           stream), ctx)
        sp.step(ptr)
        torch.cuda.synchronize()
        where = "%s B %d step %d" % ("x".join(map(str, cs)), B, t)
        for what, got in (("dyn", sp.dynamic), ("bits", sp.dynamic_bits), ("mask", sp.mask), ("cur", sp.current_mask)):
            _same(got, s[what], what + " against the two launches, " + where)
    sp.check()


@pytest.mark.parametrize("cs,B,mode", [((5, 50), 13, MODE_2D), ((12, 40), 16, MODE_2D), ((5, 5, 50), 5, MODE_3D)],
                         ids=["5x50", "12x40", "5x5x50"])
def test_outputs_at_a_16_byte_offset(T, cs, B, mode):
    """dyn_out and bits_out 16 bytes into larger guard-filled allocations (the lane roles rotate with the slab's place in
    its 64-byte granule): nothing outside the windows is written.  (dyn_out == dyn_in is refused by the entry point.)"""
    _run(T, cs, B, mode, offset=16)


def test_in_place_first_step_is_refused(T):
    L, lib = T._lib, T._lib.lib()
    B, cs = 8, (5, 50)
    static, dynamic, tape = _instance(2, B)
    st, dy, ptr = static.to(DEV), dynamic.to(DEV), tape[:, 0].contiguous().to(DEV)
    ctx, stream = L.ctx(DEV), L.stream_of(torch.device(DEV))
    env = T.BatchedContainer(B, list(cs), N, "C+P+S-lb-soft", "diff", device=DEV)
    env.reset()
    o = [torch.empty(B, 20, device=DEV) for _ in range(3)]
    bits, feat = torch.empty(B, 20, dtype=torch.int64, device=DEV), torch.empty(env._feature_shape(), device=DEV)
    rc = lib.tap_transition_first(ctx, C.byref(env.desc), L.ptr(env._state), N, 2, ROWS, 3, L.ptr(dy), L.ptr(st), st.shape[1],
                                  L.ptr(ptr), L.ptr(o[0]), L.ptr(bits), L.ptr(dy), L.ptr(o[1]), L.ptr(o[2]), L.ptr(feat), None,
                                  None, L.TAP_T_FRESH, stream)
    assert rc != 0
    torch.cuda.synchronize()
    assert torch.equal(dy.cpu(), dynamic)


@pytest.mark.parametrize("cs,B,mode", [((5, 50), 27968, MODE_2D_NT), ((5, 5, 50), 9328, MODE_3D)], ids=["2d-27968", "3d-9328"])
def test_beyond_the_write_through_limit(T, cs, B, mode):
    """The first launch whose fp32 tensor exceeds the write-through limit (64 MiB): nontemporal stores, and in 2D the
    slab-by-slab instantiation.  Against the two-launch path only, first step only."""
    _run(T, cs, B, mode, inst=_tiled(len(cs), B), oracle=False, wt=0, steps=1)
