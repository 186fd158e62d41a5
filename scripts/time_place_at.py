#!/usr/bin/env python3
"""Time the pack-net placement step (tap_env_step_at_gather, both semantics) against the LB_GREEDY step
(tap_env_step_gather) at the same shape, in one process: W = 5, B = 8 192 and 65 536, each a hipGraph of a reset and
10 gathered steps (decoder feature written; the place-at step also writes the pack-net's next input), replayed.
Prints one line per configuration and writes profiles/place_at_step.json.  Usage:

    python scripts/time_place_at.py [--reps 200] [--out profiles/place_at_step.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tap_net_amd as T  # noqa: E402

W, H, N = 5, 50, 10


def graph_of(env, static, ptr, pos_x, feat, pnet):
    def episode():
        env.reset()
        for t in range(N):
            if env.place_at is None:
                env.add_new_blocks_gather(static, ptr[t], out=feat)
            else:
                env.add_new_blocks_at_gather(static, ptr[t], pos_x[t], out=feat, pnet_out=pnet)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        episode()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        episode()
    return g


def time_graph(g, reps):
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps            # us per replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_at_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for B in (8192, 65536):
        gen = torch.Generator(device=dev).manual_seed(B)
        static = torch.zeros(B, 3, N, device=dev)
        static[:, 1, :] = torch.randint(1, W + 1, (B, N), device=dev, generator=gen).float()
        static[:, 2, :] = torch.randint(1, 5, (B, N), device=dev, generator=gen).float()
        ptr = torch.arange(N, device=dev).repeat(B, 1).t().contiguous()
        pos_x = torch.randint(0, W, (N, B), device=dev, generator=gen)
        for label, place_at in (("lb_greedy", None), ("at_container", "container"), ("at_net", "net")):
            env = T.BatchedContainer(B, [W, H], N, 'C+P+S-SL-soft', 'diff', device=dev, place_at=place_at)
            feat = env._new_feature()
            pnet = torch.empty(B, 1, W, device=dev) if place_at else None
            g = graph_of(env, static, ptr, pos_x, feat, pnet)
            us = time_graph(g, args.reps)
            row = {"step": label, "B": B, "W": W, "us_per_episode": round(us, 2), "us_per_step": round(us / N, 3),
                   "M_env_steps_per_s": round(B * N / us, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            env.check()
    out = args.out
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev), "note": "a reset + 10 steps per graph replay; "
                   "us_per_step includes the reset's share", "rows": rows}, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
