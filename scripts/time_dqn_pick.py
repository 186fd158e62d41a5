#!/usr/bin/env python3
"""Time the local pack-net's pick in one launch (tools.DQN(..., fused=True).pick; tapenv.h: tap_dqn_pick) against the PARENT
commit's package and library (DQN.forward and .max(1), stock torch), in the same session, all at W = 5, the diff form:

  - the pick alone (eager, torch.no_grad) at B = 128 and B = 8 192;
  - pack.episode_scores_net at n = 10, the same two B;
  - run_episode(pack_policy=net) captured in a hipGraph and replayed, at n = 10, B = 8 192.

Each side runs in a child process of its own that imports the package from its own tree (--parent-root: a checkout of the
parent commit with its libtapenv.so built, e.g. `git archive HEAD^ tap_net_amd.py tap-net_amd include | tar -x -C
build_prof/parent` and `make -C build_prof/parent/tap-net_amd/csrc`): device events, the median of --reps synchronised
timings after warm-up; --runs alternating runs per side; a row's spread is max - min of its side's medians.  Writes
profiles/dqn_pick.json.

Usage: python scripts/time_dqn_pick.py --parent-root build_prof/parent [--runs 3] [--reps 20]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 5, 120, 10
BATCHES = [128, 8192]
RT = 'C+P+S-SL-soft'


def child(root, fused, reps):
    sys.path.insert(0, root)
    import torch
    import tap_net_amd as T
    from tap_net_amd import synth
    dev = torch.device("cuda", 0)

    def median_us(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts)

    torch.manual_seed(0)
    net = T.tools.DQN(W, True, **({"fused": True} if fused else {})).to(dev).eval()
    rows = []
    for B in BATCHES:
        gen = torch.Generator(device=dev).manual_seed(B)
        hm = torch.randint(-6, 7, (B, 1, W), device=dev, generator=gen).float()
        blk = torch.randint(1, 6, (B, 1, 2), device=dev, generator=gen).float()
        with torch.no_grad():
            us = median_us((lambda: net.pick(hm, blk)) if fused else (lambda: net(hm, blk).max(1)))
        rows.append({"what": "pick", "B": B, "n": 1, "us": round(us, 1)})
    for B in BATCHES:
        static, dynamic = synth.rand_instances(B, N, 2, seed=N)
        tape = synth.random_feasible_tape(static, dynamic, N, seed=N + 1).to(dev)
        static = static.to(dev)
        us = median_us(lambda: T.pack.episode_scores_net(static, tape, RT, [W, H], net))
        rows.append({"what": "episode_scores_net", "B": B, "n": N, "us": round(us, 1)})
    B = BATCHES[-1]
    static, dynamic = synth.rand_instances(B, N, 2, seed=N)
    tape = synth.random_feasible_tape(static, dynamic, N, seed=N + 1).to(dev)
    static, dynamic = static.to(dev), dynamic.to(dev)
    policy = T.TapePolicy(tape)
    env = T.BatchedContainer(B, [W, H], N, RT, 'diff', device=dev, place_at='container')

    def episode():
        return T.run_episode(static, dynamic, policy, W, H, reward_type=RT, heightmap_type='diff', pack_policy=net, env=env)
    prev = T.pack._binary_mode
    T.pack.set_binary_check('trust')
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            episode()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            episode()
    finally:
        T.pack.set_binary_check(prev)
    rows.append({"what": "episode_graph", "B": B, "n": N, "us": round(median_us(g.replay), 1)})
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_pick.json"))
    ap.add_argument("--child", nargs=2, metavar=("ROOT", "FUSED"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1] == "1", args.reps)
        return
    if not args.parent_root or not os.path.exists(os.path.join(args.parent_root, "tap-net_amd", "libtapenv.so")):
        sys.exit("--parent-root must hold the parent commit's tree with its libtapenv.so built")
    sides = {"parent": (os.path.abspath(args.parent_root), "0"), "fused": (ROOT, "1")}
    runs = {k: [] for k in sides}
    for r in range(args.runs):
        for side, (root, fused) in sides.items():
            env = dict(os.environ)
            env.pop("TAP_LIB_PATH", None)                                  # each tree loads the library beside its package
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, fused, "--reps", str(args.reps)],
                               env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=600)
            if p.returncode != 0:
                sys.exit("the %s side failed with status %d" % (side, p.returncode))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")][-1]
            runs[side].append(json.loads(line[5:]))
            print(side, r, line[5:], flush=True)
    table = []
    for i, row in enumerate(runs["fused"][0]):
        out = {k: row[k] for k in ("what", "B", "n")}
        for side in sides:
            us = [run[i]["us"] for run in runs[side]]
            out[side + "_us"] = us
            out[side + "_median_us"] = statistics.median(us)
            out[side + "_spread_us"] = round(max(us) - min(us), 1)
        out["factor"] = round(out["parent_median_us"] / out["fused_median_us"], 2)
        out["faster_by_more_than_the_larger_spread"] = \
            out["parent_median_us"] - out["fused_median_us"] > max(out["parent_spread_us"], out["fused_spread_us"])
        table.append(out)
    import torch
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "W": W, "is_diff_height": True,
                   "note": "parent = the parent commit's package and library (DQN.forward and .max(1), stock torch ops); fused = this "
                           "tree, DQN(fused=True).pick, one launch per pick; device events, medians of %d synchronised calls after "
                           "warm-up, %d alternating runs per side, spread = max - min" % (args.reps, args.runs),
                   "fused_wins_every_case": all(r["faster_by_more_than_the_larger_spread"] for r in table),
                   "rows": table}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
