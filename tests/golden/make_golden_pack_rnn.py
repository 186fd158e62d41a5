#!/usr/bin/env python3
"""Generate tests/golden/pack_rnn.npz by running the UPSTREAM REFERENCE's global pack-net (reward types C+P+S-G-soft /
C+P+S-LG-soft, pack_net/LG_RL.py) on the CPU:
  - LG_RL.PackEngine traces for W in {2, 5, 7, 10, 16, 31, 64}: 25 steps (wraps after steps 10 and 20), columns beyond
    W - w, some fractional block sides; per step the position, the stability flag, the reward, valid / empty and the
    height-map before the wrap, and get_heightap in all three forms after the step;
  - LG_RL.PackRNN forwards, 'G' and 'LG', seeded random weights (the test rebuilds them from the seed), W = 5 and 10,
    blocks_num in {1, 7, 10, 12, 20} (and 7 of 12 columns): positions, hit_porb_log, -reward, get_heightap after the
    forward, and the smallest top-1 / top-2 probability margin of the case;
  - tools.calc_positions_LG_net for seeded weights and for the shipped G checkpoint (pretrain_model/G_rand_diff),
    n <= 10 and n = 15, with the forward's own reward (which differs from the replay's ratio once the engine wraps) and
    the smallest top-1 / top-2 probability margin of the forward;
  - model.DRL_RNN.forward (seeded, eval, B = 4, n = 12, 'C+P+S-G-soft'): tour_idx, pack_logp, scores and every outer
    step's decoder_dynamic.
Like make_golden.py it runs only where the reference checkout is present; while it runs, Tensor.cuda / Module.cuda are
the identity (the reference moves every tensor to the GPU) -- that patch stays here.  Usage:

    python tests/golden/make_golden_pack_rnn.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402

ENGINE_WIDTHS = (2, 5, 7, 10, 16, 31, 64)
ENGINE_STEPS = 25
FORWARD_CASES = [(W, bn, T) for W in (5, 10) for (bn, T) in ((1, 1), (7, 7), (10, 10), (12, 12), (20, 20), (7, 12))]
FORWARD_B = 6
H = 60


def seeded_rnn(LG_RL, torch, kind, W, seed):
    torch.manual_seed(seed)
    return LG_RL.PackRNN(2, 128, W, 128, W, H, 'diff', pack_net_type=kind).eval()


def rnn_seed(kind, W):
    return 1000 + 10 * W + (1 if kind == 'LG' else 0)


def draw_blocks(rs, B, T, W):
    w = rs.randint(1, min(W, 4) + 1, size=(B, T)).astype(np.float32)
    h = rs.randint(1, 6, size=(B, T)).astype(np.float32)
    frac = rs.rand(B, T) < 0.2
    h[frac] += 0.5                                                   # block.int() truncates
    return np.stack((w, h), 1)                                       # (B, 2, T)


def main():
    mods = ref_loader.load()
    if mods is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    tools, ref_pack = mods[0], mods[1]
    import torch
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, ref_loader.REFERENCE_DIR)
    try:
        from pack_net import LG_RL
        import model as ref_model
    finally:
        sys.path.remove(ref_loader.REFERENCE_DIR)
    out = {}

    # ---- PackEngine traces -----------------------------------------------------------------------------------------
    real_add = LG_RL.add_block
    for W in ENGINE_WIDTHS:
        name = "e_w%d" % W
        rs = np.random.RandomState(sum(map(ord, name)))
        n = ENGINE_STEPS
        w = rs.randint(1, W + 1, size=n).astype(np.float32)
        w[rs.rand(n) < 0.2] += 0.5
        h = rs.randint(1, 5, size=n).astype(np.float32)
        h[rs.rand(n) < 0.2] += 0.25
        xs = rs.randint(0, W + 4, size=n).astype(np.int64)           # x > W - w is clamped by the engine
        eng = LG_RL.PackEngine(W, H, 10, False)
        seen = {}

        def add(block, pos_x, container, height_map, stable, num, is_train=True):
            res = real_add(block, pos_x, container, height_map, stable, num, is_train)
            cont, hm, st, box, valid, empty, pos, num2 = res
            seen.update(stable=bool(st[int(num2) - 1]), valid=int(valid), empty=int(empty), hm=hm.copy(),
                        py_empty=int((cont != 0).sum() - (cont >= 1).sum()))
            return res
        LG_RL.add_block = add
        rec = {k: [] for k in ("pos", "stable", "rw", "valid", "empty", "hm", "full", "zero", "diff")}
        try:
            for i in range(n):
                _, rw, done, pos = eng.step(torch.tensor(int(xs[i])), torch.tensor([w[i], h[i]]))
                rec["pos"].append([int(pos[0]), int(pos[1])])
                rec["stable"].append(seen["stable"])
                rec["rw"].append(np.float64(rw))
                rec["valid"].append(seen["valid"])
                rec["empty"].append(seen["empty"])
                rec["hm"].append(np.asarray(seen["hm"], np.int64))
                for t in ("full", "zero", "diff"):
                    rec[t].append(np.array(eng.get_heightap(t), np.float64))     # 'full' is the engine's own array
        finally:
            LG_RL.add_block = real_add
        out[name + "_cs"] = np.asarray([W, H], np.int32)
        out[name + "_blocks"] = np.stack((w, h), 1)
        out[name + "_x"] = xs
        out[name + "_pos"] = np.asarray(rec["pos"], np.int64)
        out[name + "_stable"] = np.asarray(rec["stable"], np.uint8)
        out[name + "_rw"] = np.asarray(rec["rw"], np.float64)
        out[name + "_valid"] = np.asarray(rec["valid"], np.int64)
        out[name + "_empty"] = np.asarray(rec["empty"], np.int64)
        out[name + "_hm"] = np.stack(rec["hm"])
        for t in ("full", "zero", "diff"):
            out[name + "_hap_" + t] = np.stack(rec[t])

    # ---- PackRNN forwards ------------------------------------------------------------------------------------------
    fwd = []
    for kind in ('G', 'LG'):
        for (W, bn, T) in FORWARD_CASES:
            name = "f_%s_w%d_n%d_t%d" % (kind, W, bn, T)
            net = seeded_rnn(LG_RL, torch, kind, W, rnn_seed(kind, W))
            rs = np.random.RandomState(sum(map(ord, name)))
            blocks = draw_blocks(rs, FORWARD_B, T, W)
            maps = []
            hook = net.fc.register_forward_hook(lambda m, i, o: maps.append(o.detach().clone()))
            with torch.no_grad():
                positions, logp, neg_rw = net(torch.from_numpy(blocks), bn)
            hook.remove()
            top2 = torch.stack(maps).topk(2, dim=-1).values
            out[name + "_blocks"] = blocks
            out[name + "_positions"] = np.asarray(positions, np.int64)
            out[name + "_logp"] = logp.numpy()
            out[name + "_neg_reward"] = neg_rw.numpy()
            out[name + "_margin"] = np.float64((top2[..., 0] - top2[..., 1]).min().item())
            for t in ("full", "zero", "diff"):
                out[name + "_hap_" + t] = np.stack([np.asarray(e.get_heightap(t), np.float64) for e in net.engines])
            fwd.append(name)
    out["forward_cases"] = np.asarray(fwd)
    # the parameter names and shapes of both kinds (the weights are rebuilt from the seed by the test)
    for kind in ('G', 'LG'):
        sd = seeded_rnn(LG_RL, torch, kind, 5, 0).state_dict()
        out["sd_%s_keys" % kind] = np.asarray(list(sd))
        out["sd_%s_shapes" % kind] = np.asarray([",".join(str(d) for d in v.shape) for v in sd.values()])

    # ---- tools.calc_positions_LG_net -------------------------------------------------------------------------------
    real_load = torch.load
    ckpt = os.path.join(ref_loader.REFERENCE_DIR, "pretrain_model", "G_rand_diff", "actor.pt")
    calc = []
    for src in ('seeded', 'ckpt'):
        for k, n in enumerate((3, 7, 10, 15, 5, 8) if src == 'seeded' else (3, 7, 10, 15)):
            kind = 'G' if src == 'ckpt' or k % 2 == 0 else 'LG'
            rt = 'C+P+S-%s-soft' % kind
            name = "c_%s_%s_n%d" % (src, kind, n)
            rs = np.random.RandomState(sum(map(ord, name)))
            W = 5
            blocks = np.stack((rs.randint(1, W + 1, size=n), rs.randint(1, 6, size=n)), 1).astype(np.float64)
            if src == 'ckpt':
                sd = real_load(ckpt, map_location='cpu')
            else:
                sd = seeded_rnn(LG_RL, torch, kind, W, rnn_seed(kind, W)).state_dict()
            engine_rw, margins = [], []
            real_fwd = LG_RL.PackRNN.forward

            def forward(self, *a, **kw):
                maps = []
                hook = self.fc.register_forward_hook(lambda m, i, o: maps.append(o.detach().clone()))
                try:
                    res = real_fwd(self, *a, **kw)
                finally:
                    hook.remove()
                top2 = torch.stack(maps).topk(2, dim=-1).values
                margins.append(float((top2[..., 0] - top2[..., 1]).min().item()))
                engine_rw.append(res[2].numpy().copy())
                return res
            torch.load = lambda *a, **kw: sd
            LG_RL.PackRNN.forward = forward
            try:
                pos, _, st, ratio, scores = tools.calc_positions_LG_net(blocks.copy(), [W, H], rt)
            finally:
                torch.load = real_load
                LG_RL.PackRNN.forward = real_fwd
            out[name + "_blocks"] = blocks
            out[name + "_positions"] = np.asarray(pos, np.int64)
            out[name + "_stable"] = np.asarray(st, np.uint8)
            out[name + "_ratio"] = np.float64(np.asarray(ratio).reshape(-1)[0])
            out[name + "_scores"] = np.asarray([np.asarray(v).reshape(-1)[0] for v in scores], np.int64)
            out[name + "_neg_reward"] = np.float32(engine_rw[0].reshape(-1)[0])
            out[name + "_margin"] = np.float64(margins[0])
            calc.append(name)
    out["calc_cases"] = np.asarray(calc)

    # ---- DRL_RNN.forward -------------------------------------------------------------------------------------------
    B, n, W = 4, 12, 5
    rs = np.random.RandomState(4242)
    static = np.zeros((B, 3, 2 * n), np.float32)
    ids = np.arange(n, dtype=np.float32)
    wh = np.stack((rs.randint(1, W + 1, size=(B, n)), rs.randint(1, 6, size=(B, n))), 1).astype(np.float32)
    static[:, 0, :n] = ids
    static[:, 0, n:] = ids
    static[:, 1:, :n] = wh
    static[:, 1:, n:] = wh[:, ::-1]                                  # the rotated copies (pack.py layout)
    dynamic = np.zeros((B, 3 * n, 2 * n), np.float32)                # no precedence: any order is feasible
    torch.manual_seed(77)
    actor = ref_model.DRL_RNN(2, 3 * n, 128, 256, False, "bot", True, W, H, 2, "C+P+S-G-soft", "shape_heightmap", "diff",
                              "LB_GREEDY", ref_pack.update_dynamic, ref_pack.update_mask, 1, 0.1, 1.0)
    actor.pack_net = seeded_rnn(LG_RL, torch, 'G', W, 2024)
    actor.eval()
    dyn = []
    real_fwd = LG_RL.PackRNN.forward

    def forward(self, *a, **kw):
        res = real_fwd(self, *a, **kw)
        dyn.append(np.stack([np.asarray(e.get_heightap('diff'), np.float64) for e in self.engines]))
        return res
    LG_RL.PackRNN.forward = forward
    try:
        with torch.no_grad():
            tour_idx, tour_logp, pack_logp, scores = actor(torch.from_numpy(static), torch.from_numpy(dynamic),
                                                           [torch.zeros(B, 2, 1), torch.zeros(B, W - 1, 1)])
    finally:
        LG_RL.PackRNN.forward = real_fwd
    out["drl_static"] = static
    out["drl_dynamic_shape"] = np.asarray(dynamic.shape, np.int64)
    out["drl_tour_idx"] = tour_idx.numpy().astype(np.int64)
    out["drl_pack_logp"] = pack_logp.numpy()
    out["drl_scores"] = scores.numpy()
    out["drl_decoder_dynamic"] = np.stack(dyn)
    np.savez_compressed(os.path.join(HERE, "pack_rnn.npz"), **out)


if __name__ == "__main__":
    main()
