#!/usr/bin/env python3
"""Time the global pack-net's forward in one launch (tools.PackRNN(..., fused=True); tapenv.h: tap_pack_rnn_forward)
against the PARENT commit's package and library, in the same session:

  - one forward (eager, torch.no_grad) at (B 128, n 10), (B 8 192, n 10) and (B 8 192, n 20), G and LG, W = 5, 'diff';
  - run_episode(pack_rnn=G) captured in a hipGraph and replayed, at (B 128, n 10) and (B 8 192, n 20) -- the two shapes
    DESIGN 7b quotes.

Each side runs in a child process of its own that imports the package from its own tree (--parent-root: a checkout of the
parent commit with its libtapenv.so built, e.g. `git archive HEAD^ tap_net_amd.py tap-net_amd include | tar -x -C
build_prof/parent` and `make -C build_prof/parent/tap-net_amd/csrc`): device events, the median of --reps timings after warm-up; --runs alternating runs per
side; a row's spread is max - min of its side's medians.  Writes profiles/pack_rnn_forward.json.

Usage: python scripts/time_pack_rnn_forward.py --parent-root build_prof/parent [--runs 3] [--reps 20]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 5, 120
FORWARDS = [(128, 10), (8192, 10), (8192, 20)]
EPISODES = [(128, 10), (8192, 20)]


def child(root, fused, reps):
    sys.path.insert(0, root)
    import torch
    import tap_net_amd as T
    from tap_net_amd import synth
    dev = torch.device("cuda", 0)
    kw = {"fused": True} if fused else {}

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

    rows = []
    for kind in ('G', 'LG'):
        for B, n in FORWARDS:
            torch.manual_seed(0)
            net = T.tools.PackRNN(2, 128, W, 128, W, H, 'diff', pack_net_type=kind, **kw).to(dev).eval()
            gen = torch.Generator(device=dev).manual_seed(B + n)
            blocks = torch.stack((torch.randint(1, W + 1, (B, n), device=dev, generator=gen),
                                  torch.randint(1, 5, (B, n), device=dev, generator=gen)), 1).float().contiguous()
            with torch.no_grad():
                us = median_us(lambda: net(blocks, n))
            rows.append({"what": "forward", "kind": kind, "B": B, "n": n, "us": round(us, 1)})
    for B, n in EPISODES:
        static, dynamic = synth.rand_instances(B, n, 2, seed=n)
        tape = synth.random_feasible_tape(static, dynamic, n, seed=n + 1).to(dev)
        static, dynamic = static.to(dev), dynamic.to(dev)
        torch.manual_seed(0)
        net = T.tools.PackRNN(2, 128, W, 128, W, H, 'diff', pack_net_type='G', **kw).to(dev).eval()
        policy = T.TapePolicy(tape)

        def episode():
            return T.run_episode(static, dynamic, policy, W, H, reward_type='C+P+S-G-soft', heightmap_type='diff', pack_rnn=net)
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
        rows.append({"what": "episode_graph", "kind": "G", "B": B, "n": n, "us": round(median_us(g.replay), 1)})
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_rnn_forward.json"))
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
                               env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=900)
            if p.returncode != 0:
                sys.exit("the %s side failed with status %d" % (side, p.returncode))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")][-1]
            runs[side].append(json.loads(line[5:]))
            print(side, r, line[5:], flush=True)
    table = []
    for i, row in enumerate(runs["fused"][0]):
        out = {k: row[k] for k in ("what", "kind", "B", "n")}
        for side in sides:
            us = [run[i]["us"] for run in runs[side]]
            out[side + "_us"] = us
            out[side + "_median_us"] = statistics.median(us)
            out[side + "_spread_us"] = round(max(us) - min(us), 1)
        out["factor"] = round(out["parent_median_us"] / out["fused_median_us"], 2)
        out["gain_over_3_parent_spreads"] = out["parent_median_us"] - out["fused_median_us"] > 3 * out["parent_spread_us"]
        table.append(out)
    import torch
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "W": W, "heightmap_type": "diff",
                   "note": "parent = the parent commit's package and library (torch ops between n engine launches per forward); "
                           "fused = this tree, PackRNN(fused=True), one launch per forward; device events, medians of %d after "
                           "warm-up, %d alternating runs per side, spread = max - min" % (args.reps, args.runs),
                   "rows": table}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
