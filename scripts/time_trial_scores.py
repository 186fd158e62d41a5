#!/usr/bin/env python3
"""Time BatchedContainer.trial_scores (trial.hip: k_trial_scores, one launch) against its stepped form
(``stepped=True``: nR committed steps on a scratch copy of the blob, kernels the package already had) and against ONE
add_new_blocks_gather launch on the same state, at c2's shape (2D, W = 5, n = 10, B = 8 192) and c3's (3D, 5 x 5,
n = 10, B = 4 096), on the states and masks of steps 0, 4 and 8 of a greedy best-ratio episode over instances from the
device-side RAND generator.  Every figure is the median of ``--calls`` synchronised calls (host clock around the call
and a device synchronise) after ``--warmup`` warm-ups, taken in two runs.  Also one whole run_episode under
BestRatioPolicy against RandomFeasiblePolicy.  The acceptance rule is the MACS episode change's: at every shape and
step the new call is faster than the stepped form by more than the stepped form's own spread between its two runs.
Prints one line per row and a markdown table, writes profiles/trial_scores.json.  Usage:

    python scripts/time_trial_scores.py [--calls 25] [--warmup 3] [--out profiles/trial_scores.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tap_net_amd as T  # noqa: E402
from tap_net_amd import pack, synth  # noqa: E402

SHAPES = [("c2", 2, [5, 50], 10, 8192), ("c3", 3, [5, 5, 50], 10, 4096)]
REWARD = "C+P+S-lb-soft"
STEPS = (0, 4, 8)


def median_us(fn, calls, warmup, before=None):
    for _ in range(warmup):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        if before:
            before()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trial_scores.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows, episodes, ok = [], [], True
    for name, D, cs, n, B in SHAPES:
        st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
        nR = int(st.shape[2])
        env = T.BatchedContainer(B, cs, n, REWARD, "diff", device=dev)
        scratch = T.BatchedContainer(B, cs, n, REWARD, "diff", device=dev)
        masks = pack.MaskStepper(st, dy)
        out = torch.empty(B, nR, dtype=torch.float64, device=dev)
        best = torch.empty(B, dtype=torch.int64, device=dev)
        feat = scratch._new_feature()
        for step in range(max(STEPS) + 1):
            cur = masks.current_mask
            env.trial_scores(st, cur, out=out, best_out=best)
            ptr = best.clone()
            if step in STEPS:
                fused = lambda: env.trial_scores(st, cur, out=out, best_out=best)                       # noqa: E731
                stepped = lambda: env.trial_scores(st, cur, out=out, best_out=best, stepped=True)       # noqa: E731
                one_step = lambda: scratch.add_new_blocks_gather(st, ptr, out=feat)                     # noqa: E731
                restore = lambda: scratch._state.copy_(env._state)                                      # noqa: E731
                runs = []
                for _ in range(2):
                    runs.append((median_us(fused, args.calls, args.warmup), median_us(stepped, args.calls, args.warmup),
                                 median_us(one_step, args.calls, args.warmup, before=restore)))
                f, s, o = ([r[k] for r in runs] for k in range(3))
                spread = abs(s[0] - s[1])
                passed = min(s) - max(f) > spread
                ok = ok and passed
                row = {"shape": name, "D": D, "container": cs, "n": n, "B": B, "step": step,
                       "live_columns_mean": round(float(cur.sum(1).mean().item()), 2),
                       "trial_scores_us": [round(v, 1) for v in f], "stepped_us": [round(v, 1) for v in s],
                       "one_step_launch_us": [round(v, 1) for v in o], "stepped_spread_us": round(spread, 1),
                       "stepped_over_fused": round(statistics.mean(s) / statistics.mean(f), 1),
                       "fused_over_one_step": round(statistics.mean(f) / statistics.mean(o), 2), "faster_than_spread": passed}
                rows.append(row)
                print(json.dumps(row), flush=True)
            masks.step(ptr)
            env.add_new_blocks_gather(st, ptr, want_feature=False)
        env.check()
        # a whole episode on the fused stepper: the greedy policy against the mask-only random one
        eenv = T.BatchedContainer(B, cs, n, REWARD, "diff", device=dev)
        for label, policy in (("BestRatioPolicy", T.BestRatioPolicy(eenv)), ("RandomFeasiblePolicy", T.RandomFeasiblePolicy())):
            ep = lambda: T.run_episode(st, dy, policy, cs[0], cs[-1], reward_type=REWARD, env=eenv)     # noqa: E731
            us = [median_us(ep, args.episodes, 2) for _ in range(2)]
            row = {"shape": name, "B": B, "policy": label, "episode_us": [round(v, 1) for v in us]}
            episodes.append(row)
            print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev),
                   "note": "medians of %d synchronised calls after %d warm-ups, two runs each; stepped = trial_scores("
                           "stepped=True); one_step_launch = add_new_blocks_gather on the same state" % (args.calls, args.warmup),
                   "accepted": ok, "rows": rows, "episodes": episodes}, f, indent=1)
    print("| shape | step | live | trial_scores us | stepped us | one step us | stepped / fused | fused / one step |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %.1f | %s | %s | %s | %.1f | %.2f |" % (
            r["shape"], r["step"], r["live_columns_mean"], " / ".join("%.0f" % v for v in r["trial_scores_us"]),
            " / ".join("%.0f" % v for v in r["stepped_us"]), " / ".join("%.0f" % v for v in r["one_step_launch_us"]),
            r["stepped_over_fused"], r["fused_over_one_step"]))
    for r in episodes:
        print("| %s | episode | %s | %s |" % (r["shape"], r["policy"], " / ".join("%.0f" % v for v in r["episode_us"])))
    print("accepted" if ok else "NOT accepted", "- wrote", args.out)


if __name__ == "__main__":
    main()
