"""Every case of tests/stream_cases.CASES on the GPU: the launch record (tapenv.h: tap_variant_hits) holds exactly the
instantiations the restated launcher rules and the host selector predict, wt included, and after EVERY step the outputs
equal the CPU oracle's bit for bit -- the fp32 `dynamic`, its bit shadow, current_mask and mask, the feature -- and at the
end positions, stable flags and the ratio.  The C ABI cases place dyn_out 16 / 32 / 48 bytes into a larger buffer (the
lane-role rotation sb_add = 1 / 2 / 3 of write-through launches, tap_masks.h: mask_finish) and check the bytes around it."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
import stream_cases as S

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
GUARD = 256                                   # bytes checked on either side of a seam's dyn_out window
# MACS 3D on a 2 x 4 footprint (the 8-lane entries of k_transition_macs3) with these instances, whose blocks are wider than
# the container: the device raises error bits and writes features the oracle does not.  That is the MACS 3D placement,
# not the precedence update; for these cases the stream outputs and the launch record are checked, the placement is not.
PLACEMENT_UNCHECKED = lambda c: c.strategy == "MACS" and c.D == 3 and c.cells <= 8


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


@pytest.fixture(scope="module")
def sv():
    lib = S.selector()
    if lib is None:
        pytest.skip("no g++ for the host build of the selector")
    return lib


def _instances(c, seed):
    from tap_net_amd import synth
    static, dynamic = synth.rand_instances(c.B, c.n, c.D, seed=seed)
    full = dynamic
    if c.input_type == "rot":
        dynamic = dynamic[:, :c.n].contiguous()
        full = torch.cat([dynamic, torch.zeros_like(dynamic), torch.zeros_like(dynamic)], 1)
    tape = synth.random_feasible_tape(static, full, c.n, seed=seed + 3)
    return static, dynamic, tape


def _expand(bits, B, rows, nR):
    words = bits.view(B, -1, nR)
    r = torch.arange(rows, device=bits.device)
    return ((words[:, (r // 64)] >> (r % 64).view(1, -1, 1)) & 1).to(torch.float32)


def _eq(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d mismatches, first at %s: %r != %r" % (what, len(bad), bad[0].tolist(), got[tuple(bad[0])],
                                                                         want[tuple(bad[0])])


def _stepper_case(T, c):
    from tap_net_amd import pack
    env = T.BatchedContainer(c.B, list(c.cs), c.n, c.reward, "diff", packing_strategy=c.strategy, device=DEV)
    sp = None
    for ep in range(c.episodes):
        static, dynamic, tape = _instances(c, seed=c.B + 17 * ep)
        st, dy, tp = static.to(DEV), dynamic.to(DEV), tape.to(DEV)
        if sp is None:
            sp = pack.EpisodeStepper(st, dy, env, input_type=c.input_type, steps=c.nsteps, expand_dynamic=c.path != "noexpand",
                                     inplace_dynamic=c.path == "inplace")
        stn, dyn_ref, tape_np = static.numpy(), dynamic.numpy().copy(), tape.numpy()
        blocks = np.stack([stn[np.arange(c.B), 1:, tape_np[:, t]] for t in range(c.nsteps)], axis=1).astype(np.int32)
        ref = O.run_episodes(O.make_desc(list(c.cs), c.n, c.reward, "diff", c.strategy), blocks)
        T._lib.variant_hits_reset(DEV)
        sp.begin(st, dy, initial_mask=c.init_mask)
        mask = np.ones((c.B, c.nR), np.float32)
        if c.init_mask or not S.shadow_ok(c):
            _eq(sp.current_mask, O.initial_mask(dyn_ref, c.n), "initial current_mask")
            _eq(sp.mask, mask, "initial mask")
        for t in range(c.nsteps):
            p = tape_np[:, t]
            sp.step(tp[:, t].contiguous())
            dyn_ref = O.update_dynamic(dyn_ref, stn, p, c.n, c.update_rows)
            cur, mask = O.update_mask(mask, dyn_ref, p, c.n, c.R)
            where = "%s ep %d step %d" % (c.name, ep, t)
            if c.path != "noexpand":
                _eq(sp.dynamic, dyn_ref, "dynamic, " + where)
            if S.shadow_ok(c):
                _eq(_expand(sp.dynamic_bits, c.B, c.rows, c.nR), dyn_ref, "bit shadow, " + where)
            _eq(sp.current_mask, cur, "current_mask, " + where)
            _eq(sp.mask, mask, "mask, " + where)
            if not PLACEMENT_UNCHECKED(c):
                _eq(sp.decoder_dynamic.reshape(c.B, -1).to(torch.int64), ref["features"][:, t], "feature, " + where)
        torch.cuda.synchronize()
        if PLACEMENT_UNCHECKED(c):
            yield ep
            continue
        for what, got, want in (("positions", env.positions, ref["positions"]), ("stable", env.stable, ref["stable"].astype(bool))):
            want = want.reshape(c.B, -1)                        # the oracle ran the episode's steps only
            _eq(got.reshape(c.B, -1)[:, :want.shape[1]], want, what + ", " + c.name)
        # a container whose blocks do not fit raises an error bit; its ratio is then undefined (reward NaN-flagged,
        # rollout._flagged_reward) and only the flag is compared
        bad = ref["errs"].reshape(c.B) != 0
        _eq(env.errors.cpu().numpy() != 0, bad, "error flags, " + c.name)
        got_r, want_r = sp.ratio.cpu().numpy()[~bad], ref["ratio"].astype(np.float32)[~bad]
        assert np.array_equal(got_r, want_r, equal_nan=True), "ratio, %s: %s != %s" % (c.name, got_r, want_r)
        yield ep
    pack.check_binary()                                    # (container errors are compared with the oracle's above)


def _seam_case(T, c):
    """One step through a C ABI entry point (tap_mask_step_bits, tap_mask_step, tap_transition, tap_transition_bits) with
    dyn_out `offset` bytes into a guarded buffer."""
    from tap_net_amd import pack
    L, lib = T._lib, T._lib.lib()
    static, dynamic, tape = _instances(c, seed=c.B + 5)
    st, dy = static.to(DEV), dynamic.to(DEV)
    shadow = S.shadow_ok(c)
    bits_in = pack.dynamic_bits(dy)[0] if shadow else None
    bits_out = torch.empty_like(bits_in) if shadow else None
    numel = c.B * c.rows * c.nR
    pad = GUARD // 4
    buf = torch.full((2 * pad + numel + 16,), 7.25, dtype=torch.float32, device=DEV)
    base = buf.data_ptr()
    assert base % 64 == 0
    start = (pad * 4 + c.offset) // 4
    dyn_out = buf[start:start + numel]
    assert ((dyn_out.data_ptr() >> 4) & 3) == c.offset // 16
    ptr = tape[:, 0].to(DEV).contiguous()
    cur = torch.empty(c.B, c.nR, device=DEV)
    new = torch.empty(c.B, c.nR, device=DEV)
    mask_in = torch.ones(c.B, c.nR, device=DEV)
    ctx, stream = L.ctx(DEV), L.stream_of(torch.device(DEV))
    cs_in = pack.dynamic_colsum(dy, c.n) if c.path in ("seam_mask_step", "seam_transition") else None
    cs_out = torch.empty_like(cs_in) if cs_in is not None else None
    env = feat = None
    if c.path in ("seam_transition", "seam_transition_bits"):
        env = T.BatchedContainer(c.B, list(c.cs), c.n, c.reward, "diff", packing_strategy=c.strategy, device=DEV)
        feat = torch.empty(env._feature_shape(), device=DEV)
    L.variant_hits_reset(DEV)
    if c.path == "seam_bits":
        L.check(lib.tap_mask_step_bits(ctx, c.B, c.n, c.R, c.rows, c.update_rows, L.ptr(bits_in), L.ptr(st), st.shape[1],
                                       L.ptr(ptr), L.ptr(mask_in), L.ptr(bits_out), dyn_out.data_ptr(), L.ptr(cur),
                                       L.ptr(new), stream), ctx)
    elif c.path == "seam_mask_step":
        L.check(lib.tap_mask_step(ctx, c.B, c.n, c.R, c.rows, c.update_rows, L.ptr(dy), L.ptr(st), st.shape[1], L.ptr(ptr),
                                  L.ptr(mask_in), L.ptr(cs_in), dyn_out.data_ptr(), L.ptr(cs_out), L.ptr(cur), L.ptr(new),
                                  stream), ctx)
    elif c.path == "seam_transition":
        L.check(lib.tap_transition(ctx, C.byref(env.desc), L.ptr(env._state), c.n, c.R, c.rows, c.update_rows, L.ptr(dy),
                                   L.ptr(st), st.shape[1], L.ptr(ptr), L.ptr(mask_in), L.ptr(cs_in), dyn_out.data_ptr(),
                                   L.ptr(cs_out), L.ptr(cur), L.ptr(new), L.ptr(feat), None, L.TAP_T_FRESH, stream), ctx)
    elif c.path == "seam_transition_bits":
        L.check(lib.tap_transition_bits(ctx, C.byref(env.desc), L.ptr(env._state), c.n, c.R, c.rows, c.update_rows,
                                        L.ptr(bits_in), L.ptr(st), st.shape[1], L.ptr(ptr), L.ptr(mask_in), L.ptr(bits_out),
                                        dyn_out.data_ptr(), L.ptr(cur), L.ptr(new), L.ptr(feat), None, L.TAP_T_FRESH,
                                        stream), ctx)
    else:
        raise AssertionError("no runner for path %r" % c.path)
    torch.cuda.synchronize()
    stn, p = static.numpy(), tape.numpy()[:, 0]
    dyn_ref = O.update_dynamic(dynamic.numpy(), stn, p, c.n, c.update_rows)
    want_cur, want_mask = O.update_mask(np.ones((c.B, c.nR), np.float32), dyn_ref, p, c.n, c.R)
    _eq(dyn_out.view(c.B, c.rows, c.nR), dyn_ref, "dynamic, " + c.name)
    if c.path in ("seam_bits", "seam_transition_bits"):
        _eq(_expand(bits_out, c.B, c.rows, c.nR), dyn_ref, "bit shadow, " + c.name)
    _eq(cur, want_cur, "current_mask, " + c.name)
    _eq(new, want_mask, "mask, " + c.name)
    _eq(buf[:start], np.full(start, 7.25, np.float32), "bytes before dyn_out, " + c.name)
    _eq(buf[start + numel:], np.full(buf.numel() - start - numel, 7.25, np.float32), "bytes after dyn_out, " + c.name)
    if feat is not None and not PLACEMENT_UNCHECKED(c):
        blocks = stn[np.arange(c.B), 1:, p][:, None, :].astype(np.int32)
        ref = O.run_episodes(O.make_desc(list(c.cs), c.n, c.reward, "diff", c.strategy), blocks)
        _eq(feat.reshape(c.B, -1).to(torch.int64), ref["features"][:, 0], "feature, " + c.name)
    yield 0


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_case_against_the_oracle(T, sv, case):
    want = S.keys(sv, S.launches(case))
    run = _seam_case if case.path.startswith("seam") else _stepper_case
    for _ in run(T, case):
        got = T._lib.variant_keys(DEV)
        assert got == want, "launched %s, predicted %s" % (sorted(got - want), sorted(want - got))
