#!/usr/bin/env python3
"""Time the global pack-net's loop (DRL_RNN without its pointer network: run_episode(..., pack_rnn=net)) and its
engine step (tap_env_step_engine), in one process:
  - episodes: a tools.PackRNN ('G', eval, 'diff', random weights) re-packs every prefix, n (n + 1) / 2 engine launches
    per episode; W = 5, n = 10 and 20, B = 128 and 8 192, each episode captured in a hipGraph and replayed;
  - steps: a hipGraph of 10 engine steps (next input and reward written) against a reset and 10 place-at steps with
    TAP_AT_NET's rules (tap_env_step_at, next input written, as scripts/time_place_at.py times them) at W = 5,
    B = 8 192, replayed.
Writes profiles/pack_rnn_episode.json.  The engine kernel's own time comes from a profiler pass over --engine-only
(eager engine steps, nothing else on the device), folded into the same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o pack_rnn -- \
        python scripts/time_pack_rnn.py --engine-only
    python scripts/time_pack_rnn.py --stats-csv OUT/.../pack_rnn_kernel_stats.csv

Usage: python scripts/time_pack_rnn.py [--reps 20] [--out profiles/pack_rnn_episode.json]
"""
import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tap_net_amd as T  # noqa: E402
from tap_net_amd import synth  # noqa: E402

W, H, STEPS = 5, 120, 10


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        fn()
    return g


def time_graph(g, reps):
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps            # us per replay


def step_inputs(B, dev):
    gen = torch.Generator(device=dev).manual_seed(B)
    blocks = torch.stack((torch.randint(1, W + 1, (B, STEPS), device=dev, generator=gen),
                          torch.randint(1, 5, (B, STEPS), device=dev, generator=gen)), 1).float().contiguous()
    xs = torch.randint(0, W, (STEPS, B), device=dev, generator=gen)
    return blocks, xs


def time_steps(B, reps, dev):
    blocks, xs = step_inputs(B, dev)
    eng = T.env.PackEngines(B, W, H, STEPS, 'diff', max_blocks_num=10, device=dev)
    feat = eng.env._new_feature()
    g_eng = capture(lambda: [eng.step(i, blocks, xs[i], out=feat) for i in range(STEPS)])
    env = T.BatchedContainer(B, [W, H], STEPS, 'C+P+S-G-soft', 'diff', device=dev, place_at='net')
    pnet = torch.empty(B, 1, W, device=dev)
    bt = blocks.transpose(1, 2).contiguous()                  # (B, STEPS, 2)
    cols = [bt[:, i].contiguous() for i in range(STEPS)]

    def at_net():
        env.reset()
        for i in range(STEPS):
            env.add_new_blocks_at(cols[i], xs[i], want_feature=False, pnet_out=pnet)
    g_at = capture(at_net)
    rows = []
    for label, g, note in (("engine", g_eng, "10 engine steps, next input and reward written"),
                           ("at_net", g_at, "a reset + 10 TAP_AT_NET steps, next input written")):
        us = time_graph(g, reps * 10)
        rows.append({"step": label, "B": B, "W": W, "us_per_replay": round(us, 2), "us_per_step": round(us / STEPS, 3),
                     "note": note})
        print(json.dumps(rows[-1]), flush=True)
    eng.check()
    env.check()
    return rows


def time_episode(B, n, reps, dev):
    static, dynamic = synth.rand_instances(B, n, 2, seed=n)
    tape = synth.random_feasible_tape(static, dynamic, n, seed=n + 1).to(dev)
    static, dynamic = static.to(dev), dynamic.to(dev)
    torch.manual_seed(0)
    net = T.tools.PackRNN(2, 128, W, 128, W, H, 'diff', pack_net_type='G').to(dev).eval()
    policy = T.TapePolicy(tape)
    prev = T.pack._binary_mode
    T.pack.set_binary_check('trust')
    try:
        g = capture(lambda: T.run_episode(static, dynamic, policy, W, H, reward_type='C+P+S-G-soft',
                                          heightmap_type='diff', pack_rnn=net))
    finally:
        T.pack.set_binary_check(prev)
    us = time_graph(g, reps)
    row = {"episode": "run_episode(pack_rnn=G)", "B": B, "W": W, "n": n, "engine_launches": n * (n + 1) // 2,
           "us_per_episode": round(us, 1), "M_outer_steps_per_s": round(B * n / us, 3)}
    print(json.dumps(row), flush=True)
    return row


def engine_only(dev):
    """eager engine steps for a profiler pass: B = 8 192, W = 5, 200 steps"""
    B = 8192
    blocks, xs = step_inputs(B, dev)
    eng = T.env.PackEngines(B, W, H, STEPS, 'diff', max_blocks_num=10, device=dev)
    feat = eng.env._new_feature()
    for _ in range(20):
        for i in range(STEPS):
            eng.step(i, blocks, xs[i], out=feat)
    torch.cuda.synchronize()
    eng.check()


def fold_stats(path, out):
    """the profiler's per-kernel statistics of k_place_at (the engine instantiation is k_place_at<G, true, true>)"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "k_place_at" in r.get("Name", ""):
                rows.append({"kernel": r["Name"], "calls": int(r["Calls"]),
                             "average_us": round(float(r["AverageNs"]) / 1e3, 3),
                             "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)})
    with open(out) as f:
        prof = json.load(f)
    prof["kernel_stats"] = {"source": "rocprofv3 --kernel-trace --stats over --engine-only (B = 8192, W = 5, eager)",
                            "rows": rows}
    with open(out, "w") as f:
        json.dump(prof, f, indent=1)
    print(json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_rnn_episode.json"))
    ap.add_argument("--engine-only", action="store_true")
    ap.add_argument("--stats-csv")
    args = ap.parse_args()
    if args.stats_csv:
        fold_stats(args.stats_csv, args.out)
        return
    dev = torch.device("cuda", 0)
    if args.engine_only:
        engine_only(dev)
        return
    steps = time_steps(8192, args.reps, dev)
    episodes = [time_episode(B, n, args.reps, dev) for B in (128, 8192) for n in (10, 20)]
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev), "note": "hipGraph replays; an episode re-packs every "
                   "prefix (n (n + 1) / 2 engine launches) and runs the G PackRNN between them",
                   "steps": steps, "episodes": episodes}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
