"""Every case of tests/episode_rolling_cases.CASES on the GPU.  The launch record (tapenv.h: tap_variant_hits) on the
whole-episode and rolling kinds (16 .. 21) holds exactly the keys the restated rules predict, wt included; the stream-wave
kinds, which the last window of a rolling episode also launches, are checked by tests/test_stream_variants_gpu.py.  Then
the results equal the CPU oracle's bit for bit:
  episodes   pack.reward against O.reward; pack.episode_scores (target None, 0, 1) and generate.pack_blocks against
             tools.calc_positions_lb_greedy / calc_positions_mcs per container: fp64 ratio, scores, fp32 reward,
             positions, stable flags, and which containers raised an error;
  rolling    after every one-step window the static and dynamic tensors and current_mask against O.Rolling; at the end
             the packing, height-map and ratio against O.Env (error flags against its add_new_block return codes); the
             fused path against fused=False over the whole batch;
  raw step   one tap_rolling_step into guarded buffers: the next window against O.Rolling and no byte written past
             instance B - 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_rolling_cases as S
import oracle_lib as O

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
GUARD = 64                                    # elements after each raw-step output that must stay untouched


@pytest.fixture(scope="module")
def T():
    import tap_net_amd
    return tap_net_amd


def _record(T):
    return {k for k in T._lib.variant_keys(DEV) if k[0] in S.KINDS}


def _check_record(T, c):
    got, want = _record(T), S.launches(c)
    assert got == want, "%s: launched %s, predicted %s" % (c.name, sorted(got - want), sorted(want - got))


def _eq(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s != %s" % (what, got.shape, want.shape)
    if np.array_equal(got, want, equal_nan=got.dtype.kind == "f"):
        return
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    assert False, "%s: %d mismatches, first at %s: %r != %r" % (what, len(bad), bad[0].tolist(), got[tuple(bad[0])],
                                                                 want[tuple(bad[0])])


# ---- episodes ---------------------------------------------------------------------------------------------------------
def _blocks(c, rng):
    """(B, n, D) block sides: within the container's base (heights 1 .. 5), or up to 2 wider where the case overflows.
    MACS 3D blocks stay within the container sides (the device rejects wider ones on purpose, tap_macs3.h)."""
    D, W, L = S.sides(c.cs)
    grow = 2 if c.overflow and not (c.strategy == "MACS" and D == 3) else 0
    b = np.empty((c.B, c.n, D), np.int32)
    b[:, :, 0] = rng.integers(1, W + 1 + grow, (c.B, c.n))
    if D == 3:
        b[:, :, 1] = rng.integers(1, L + 1 + grow, (c.B, c.n))
    b[:, :, -1] = rng.integers(1, 6, (c.B, c.n))
    return b


def _episode_case(T, c):
    from tap_net_amd import generate, pack
    rng = np.random.default_rng(c.B * 1000 + c.n)
    blocks = _blocks(c, rng)
    D = c.D
    W, H = c.cs[0], c.cs[-1]
    if c.entry == "pack_blocks":
        T._lib.variant_hits_reset(DEV)
        pos, st, rew = generate.pack_blocks(torch.from_numpy(blocks).to(DEV), list(c.cs), c.reward)
        torch.cuda.synchronize()
        _check_record(T, c)
        pos, st, rew = pos.cpu().numpy(), st.cpu().numpy(), rew.cpu().numpy()
        for b in range(c.B):
            rc, p, s, ratio, _ = O.calc_positions_lb_greedy(blocks[b], list(c.cs), c.reward)
            where = "%s instance %d" % (c.name, b)
            assert np.isnan(rew[b]) == (rc != 0), "error flag, " + where
            if rc == 0:
                _eq(pos[b], p, "positions, " + where)
                _eq(st[b], s, "stable, " + where)
                assert rew[b] == -np.float32(ratio), "reward, %s: %r != %r" % (where, rew[b], -np.float32(ratio))
        return
    # static (B, 1 + D [+ target], n) of the 'bot' / 'mul' input types without rotations, and a random tour
    mul = c.target is not None
    static = np.zeros((c.B, 1 + D + int(mul), c.n), np.float32)
    static[:, 0] = np.arange(c.n)
    static[:, 1:1 + D] = blocks.transpose(0, 2, 1)
    if mul:
        static[:, -1] = rng.integers(0, 2, (c.B, c.n))
    tour = np.argsort(rng.random((c.B, c.n)), axis=1).astype(np.int64)
    st, tr = torch.from_numpy(static).to(DEV), torch.from_numpy(tour).to(DEV)
    T._lib.variant_hits_reset(DEV)
    if c.entry == "reward":
        got = pack.reward(st, tr, c.reward, "bot", False, W, H)
        torch.cuda.synchronize()
        _check_record(T, c)
        nerr, want = O.reward(static, tour, c.reward, W, H)
        # a container that overflowed reports NaN (rollout._flagged_reward); the oracle's error words name the same set
        order = np.stack([static[b][1:, tour[b]].T for b in range(c.B)]).astype(np.int32)
        bad = O.run_episodes(O.make_desc(list(c.cs[:1]) * (D - 1) + [H], c.n, c.reward, "full"), order)["errs"] != 0
        got = got.cpu().numpy()
        assert nerr == bad.sum() and (bad.any() == c.overflow or not c.overflow), (c.name, nerr)
        _eq(np.isnan(got), bad, "error flags, " + c.name)
        _eq(got[~bad], want[~bad], "reward, " + c.name)
        return
    ratio, scores = pack.episode_scores(st, tr, c.reward, "mul" if mul else "bot", False, list(c.cs), c.strategy,
                                        target=c.target, check=False)
    torch.cuda.synchronize()
    _check_record(T, c)
    ratio, scores = ratio.cpu().numpy(), scores.cpu().numpy()
    calc = O.calc_positions_mcs if c.strategy == "MACS" else O.calc_positions_lb_greedy
    for b in range(c.B):
        order = static[b][:, tour[b]]
        mine = order[1:1 + D].T.astype(np.int32)
        if mul:
            mine = mine[order[-1] == c.target]
        where = "%s instance %d" % (c.name, b)
        if len(mine) == 0:                                 # pack.py:760-769: an empty list scores zeros
            assert ratio[b] == 0 and not scores[b].any(), "empty list, " + where
            continue
        rc, _, _, want_r, want_s = calc(mine, list(c.cs), c.reward)
        assert np.isnan(ratio[b]) == (rc != 0), "error flag, %s: ratio %r, oracle rc %d" % (where, ratio[b], rc)
        if rc == 0:
            assert ratio[b] == want_r, "ratio, %s: %r != %r" % (where, ratio[b], want_r)
            _eq(scores[b], want_s, "scores, " + where)


# ---- rolling ----------------------------------------------------------------------------------------------------------
def _instances(c, seed):
    """(blocks, positions) (B, N, D) of packed initial containers of side c.init: generated, or unit blocks on a grid."""
    from tap_net_amd import generate as gen
    D, N = c.D, c.n
    if c.grid:
        w = c.init[0]
        i = np.arange(N)
        pos = np.stack([i % w, i // w % w, i // (w * w)] if D == 3 else [i % w, i // w], 1).astype(np.int32)
        assert pos[:, -1].max() < c.init[-1]
        blocks = torch.ones(c.B, N, D, dtype=torch.int32, device=DEV)
        return blocks, torch.from_numpy(np.broadcast_to(pos, (c.B, N, D)).copy()).to(DEV)
    if N <= 64:
        _, _, blocks, positions = gen.generate_instances(c.B, N, D, c.init[0], c.init[-1], 1, (1, min(5, c.init[0] + 1)),
                                                         seed=seed, device=DEV, return_aux=True)
        return blocks, positions
    # above 64 blocks (the generator's precedence tensors stop there): random layers, each filled with blocks of the
    # layer's height whose sides tile the base, so every block rests on a full layer
    rng = np.random.default_rng(seed)
    w = c.init[0]
    blocks = np.zeros((c.B, N, D), np.int32)
    pos = np.zeros((c.B, N, D), np.int32)
    for b in range(c.B):
        k, z = 0, 0
        while k < N:
            h, y = int(rng.integers(1, 4)), 0
            while y < (w if D == 3 else 1) and k < N:
                d, x = (int(rng.integers(1, min(4, w - y) + 1)) if D == 3 else 1), 0
                while x < w and k < N:
                    bw = int(rng.integers(1, min(4, w - x) + 1))
                    blocks[b, k], pos[b, k] = ((bw, d, h), (x, y, z)) if D == 3 else ((bw, h), (x, z))
                    x, k = x + bw, k + 1
                y += d
            z += h
        assert z <= c.init[-1], c.name
    return torch.from_numpy(blocks).to(DEV), torch.from_numpy(pos).to(DEV)


class _Policy:
    """Random feasible picks from a seeded generator; with `check`, every window of the sampled instances against
    O.Rolling and every pick into an O.Env, as the episode goes."""

    def __init__(self, c, blocks, positions, idx, check):
        self.c, self.idx, self.check = c, idx, check
        self.g = torch.Generator(device=DEV)
        self.g.manual_seed(c.B + c.n)
        if check:
            bl, ps = blocks.cpu().numpy(), positions.cpu().numpy()
            self.ro = [O.Rolling(bl[b], ps[b], list(c.init), c.child) for b in idx]
            self.env = [O.Env(list(c.cs), c.n, c.reward, "diff") for _ in idx]
            self.err = np.zeros(len(idx), bool)
            self.last = [None] * len(idx)

    def __call__(self, step, static, dynamic, current_mask, **_):
        ptr = torch.multinomial(current_mask, 1, generator=self.g).squeeze(1)
        if not self.check:
            return ptr
        c, sel = self.c, torch.tensor(self.idx, device=DEV)
        st, dy = static[sel].cpu().numpy(), dynamic[sel].cpu().numpy()
        cm, p = current_mask[sel].cpu().numpy(), ptr[sel].cpu().numpy()
        one_step = step < c.n - c.child
        for j, b in enumerate(self.idx):
            where = "%s instance %d step %d" % (c.name, b, step)
            if step <= c.n - c.child:
                rc, ost, ody, _ = self.ro[j].convert_to_input()
                assert rc == (0 if one_step else 1), "window count, " + where
                _eq(st[j], ost, "static, " + where)
                _eq(dy[j], ody, "dynamic, " + where)
                if one_step:
                    _eq(cm[j], O.initial_mask(ody[None], c.child)[0], "current_mask, " + where)
                    self.ro[j].remove(int(p[j]) % c.child)
                else:
                    self.last[j] = ost
            else:
                _eq(st[j], self.last[j], "static of the last window, " + where)
            rc, _ = self.env[j].add_new_block(st[j][1:, int(p[j])])
            self.err[j] |= rc != 0
        return ptr


def _sample(c):
    if not c.sample:
        return list(range(c.B))
    return sorted(set(np.linspace(0, c.B - 1, c.sample).astype(int).tolist()) | {c.B - 1})


def _rolling_case(T, c):
    blocks, positions = _instances(c, seed=c.B + c.n)
    W, H = c.cs[0], c.cs[-1]
    idx = _sample(c)
    outs = {}
    for fused in ((True, False) if c.entry == "rolling" else (False, True)):
        pol = _Policy(c, blocks, positions, idx, check=not outs)
        T._lib.variant_hits_reset(DEV)
        out = T.run_rolling_episode(blocks, positions, list(c.init), pol, W, H, child_graph_size=c.child,
                                    reward_type=c.reward, fused=fused)
        torch.cuda.synchronize()
        if not outs:
            _check_record(T, c)
            first = pol
        outs[fused] = out
    a, b = outs[c.entry == "rolling"], outs[c.entry != "rolling"]
    for k in ("tour_idx", "nodes", "reward"):
        _eq(a[k], b[k].cpu().numpy(), "fused against fused=False, %s, %s" % (k, c.name))
    for k in ("positions", "errors", "heightmap"):
        _eq(getattr(a["env"], k), getattr(b["env"], k).cpu().numpy(), "fused against fused=False, %s, %s" % (k, c.name))
    env, reward = a["env"], a["reward"].cpu().numpy()
    errors = env.errors.cpu().numpy()
    pos, hm = env.positions.cpu().numpy(), env.heightmap.cpu().numpy().reshape(c.B, -1)
    a["windows"].check()
    for j, inst in enumerate(idx):
        e, where = first.env[j], "%s instance %d" % (c.name, inst)
        assert (errors[inst] != 0) == first.err[j], "error flag, %s: device %d" % (where, errors[inst])
        if first.err[j]:
            assert np.isnan(reward[inst]), "reward of a container with an error, " + where
            continue
        _eq(pos[inst].reshape(-1, c.D), e.positions, "positions, " + where)
        _eq(hm[inst], e.heightmap.reshape(-1), "height-map, " + where)
        assert np.float32(e.calc_ratio()) == -reward[inst], "ratio, %s: %r != %r" % (where, e.calc_ratio(), -reward[inst])


def _guarded(n, dtype, fill):
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _raw_step_case(T, c):
    from tap_net_amd import rolling
    from tap_net_amd.env import BatchedContainer
    L, lib = T._lib, T._lib.lib()
    blocks, positions = _instances(c, seed=c.B + 3)
    D, N, child, B = c.D, c.n, c.child, c.B
    R = 2 if D == 2 else 6
    nRc = child * R
    rw = rolling.RollingWindows(blocks, positions, list(c.init), child)
    win = rw.next(None)
    env = BatchedContainer(B, list(c.cs), N, c.reward, "diff", packing_strategy="LB_GREEDY", device=DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(c.B)
    ptr = torch.multinomial(win["current_mask"], 1, generator=g).squeeze(1).contiguous()
    st_buf, st_next = _guarded(B * (1 + D) * nRc, torch.float32, 7.25)
    dy_buf, dyn = _guarded(B * 3 * child * nRc, torch.float32, 7.25)
    cm_buf, cur = _guarded(B * nRc, torch.float32, 7.25)
    nd_buf, nodes = _guarded(B * child, torch.int32, -7)
    err = torch.zeros(B, dtype=torch.int32, device=DEV)
    feat = env._new_feature()
    ctx = L.ctx(DEV)
    static_cur = win["static"].contiguous()
    L.variant_hits_reset(DEV)
    L.check(lib.tap_rolling_step(ctx, C.byref(env.desc), L.ptr(env._state), N, child, L.ptr(rw.blocks), L.ptr(rw.rel),
                                 L.ptr(rw.state), L.ptr(ptr), L.ptr(static_cur), L.ptr(st_next), L.ptr(dyn), None, None,
                                 L.ptr(cur), L.ptr(nodes), L.ptr(err), L.ptr(feat), L.stream_of(torch.device(DEV))), ctx)
    torch.cuda.synchronize()
    _check_record(T, c)
    for buf, n, fill, what in ((st_buf, st_next.numel(), 7.25, "static_next"), (dy_buf, dyn.numel(), 7.25, "dynamic_out"),
                               (cm_buf, cur.numel(), 7.25, "current_mask_out"), (nd_buf, nodes.numel(), -7, "nodes_out")):
        _eq(buf[n:], np.full(GUARD, fill, buf.cpu().numpy().dtype), "bytes past instance B - 1 of %s, %s" % (what, c.name))
    bl, ps, p = blocks.cpu().numpy(), positions.cpu().numpy(), ptr.cpu().numpy()
    st0 = static_cur.cpu().numpy()
    st_next, dyn = st_next.view(B, 1 + D, nRc).cpu().numpy(), dyn.view(B, 3 * child, nRc).cpu().numpy()
    cur, nodes = cur.view(B, nRc).cpu().numpy(), nodes.view(B, child).cpu().numpy()
    pos = env.positions.cpu().numpy()
    for b in range(B):
        where = "%s instance %d" % (c.name, b)
        ro, e = O.Rolling(bl[b], ps[b], list(c.init), child), O.Env(list(c.cs), N, c.reward, "diff")
        rc, ost, _, _ = ro.convert_to_input()
        _eq(st0[b], ost, "first window, " + where)
        rc_e, _ = e.add_new_block(ost[1:, int(p[b])])
        ro.remove(int(p[b]) % child)
        rc, ost, ody, onodes = ro.convert_to_input()
        _eq(st_next[b], ost, "static_next, " + where)
        _eq(dyn[b], ody, "dynamic_out, " + where)
        _eq(cur[b], O.initial_mask(ody[None], child)[0], "current_mask_out, " + where)
        _eq(nodes[b], onodes, "nodes_out, " + where)
        if rc_e == 0:
            _eq(pos[b].reshape(-1, D)[:1], e.positions[:1], "placement, " + where)


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_case_against_the_oracle(T, case):
    if case.entry in ("reward", "scores", "pack_blocks"):
        _episode_case(T, case)
    elif case.entry == "raw_step":
        _raw_step_case(T, case)
    else:
        _rolling_case(T, case)
