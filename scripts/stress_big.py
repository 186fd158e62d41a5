#!/usr/bin/env python3
"""Randomised parity sweep of LB_GREEDY on containers of 4 097 .. 16 384 cells (big.hip: one workgroup per container)
against the CPU oracle: random 3D shapes (W * L in (4 096, 16 384]), block side ranges (incl. the 9 .. 16 wide
stability path), heights, rewards (soft / hard, C+P / C+P+S) and feature types; per configuration, every step's
features and height-maps, then positions, stable flags, counters and the fp64 ratio of every container, and the
whole-episode kernel (generate.pack_blocks) against the same oracle episodes.  2D widths above 4 096 are beyond the
oracle (its 2D support arrays stop at 4 096 columns): for them the stepped and whole-episode paths are compared with
each other (`selfcheck` in the summary).

    python scripts/stress_big.py 500 [out.json]

Prints one CASE line per configuration that disagrees and a final JSON summary (also written to out.json)."""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O                 # noqa: E402
import tap_net_amd as T                # noqa: E402
from tap_net_amd import generate as gen  # noqa: E402
DEV = "cuda:0"


def config(seed):
    rs = np.random.RandomState(5000 + seed)
    reward = str(rs.choice(["C+P+S-lb-soft", "C+P+S-lb-hard", "C+P-lb-soft", "C+P-lb-hard"]))
    feat = str(rs.choice(["diff", "zero", "full"]))
    if seed % 10 == 9:                                     # 2D above the oracle's width: self-consistency only
        W = int(rs.randint(4097, 16385)); cs = [W, int(rs.choice([20, 40, 60]))]
        lo = int(rs.randint(1, 400)); hi = lo + int(rs.randint(1, 3000))
    else:
        while True:
            W, L = int(rs.randint(20, 400)), int(rs.randint(11, 400))
            if 4096 < W * L <= 16384:
                break
        cs = [W, L, int(rs.choice([20, 30, 40, 60]))]
        lo = int(rs.randint(1, 10)); hi = int(min(17, lo + rs.randint(1, 12)))
    B = int(rs.randint(1, 40)); n = int(rs.randint(3, 9))
    return cs, n, reward, feat, B, lo, hi, int(rs.randint(2, 7)), rs


def one(seed):
    cs, n, reward, feat, B, lo, hi, hmax, rs = config(seed)
    D = len(cs)
    blocks = rs.randint(lo, hi, size=(B, n, D)).astype(np.int32)
    blocks[:, :, -1] = rs.randint(1, hmax, size=(B, n))
    blk = torch.as_tensor(blocks, device=DEV)
    env = T.BatchedContainer(B, cs, n, reward, feat, device=DEV)
    feats, hms = [], []
    for t in range(n):
        feats.append(env.add_new_blocks(blk[:, t].contiguous()).cpu().numpy().reshape(B, -1).astype(np.int64))
        hms.append(env.heightmap.cpu().numpy().reshape(B, -1))
    pos = env.positions.cpu().numpy(); st = env.stable.cpu().numpy().astype(np.uint8)
    r = env.calc_ratios64().cpu().numpy()
    epos, est, erew = gen.pack_blocks(blk, cs, reward)
    epos, est = epos.cpu().numpy(), est.cpu().numpy().astype(np.uint8)
    if D == 2:
        bad = ~((epos == pos).all((1, 2)) & (est == st).all(1))
        return cs, B * n, int(bad.sum()), 0, False
    ref = O.run_episodes(O.make_desc(cs, n, reward, feat), blocks, nthreads=8)
    good = ref["errs"] == 0
    ok = (pos == ref["positions"]).all((1, 2)) & (st == ref["stable"]).all(1) & (r == ref["ratio"])
    ok &= (env.valid_size.cpu().numpy() == ref["counters"][:, 0]) & (env.empty_size.cpu().numpy() == ref["counters"][:, 1])
    for t in range(n):
        ok &= (feats[t] == ref["features"][:, t]).all(1) & (hms[t] == ref["heightmaps"][:, t]).all(1)
    ok &= (epos == ref["positions"]).all((1, 2)) & (est == ref["stable"]).all(1)
    ok |= ~good                                            # the reference raises there: only the flag is compared
    flagged = env.errors.cpu().numpy() != 0
    ok &= flagged == ~good
    return cs, B * n, int((~ok).sum()), int((~good).sum()), True


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    t0 = time.time()
    s = dict(configurations=0, oracle_configurations=0, selfcheck_configurations=0, env_steps=0, mismatching_envs=0,
             envs_oracle_flags=0)
    for seed in range(N):
        cs, steps, bad, flags, oracle = one(seed)
        s["configurations"] += 1
        s["oracle_configurations" if oracle else "selfcheck_configurations"] += 1
        s["env_steps"] += steps; s["mismatching_envs"] += bad; s["envs_oracle_flags"] += flags
        if bad:
            print("CASE", seed, cs, config(seed)[1:8], "mismatching envs", bad, flush=True)
    s["seconds"] = round(time.time() - t0, 1)
    print(json.dumps(s))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(s, f, indent=1)


if __name__ == "__main__":
    main()
