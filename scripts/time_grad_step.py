#!/usr/bin/env python3
"""Time one eager decoding step of pack.EpisodeStepper at c2 (2D, W = 5, n = 10, B = 8 192) under ``torch.no_grad()`` and
with grad enabled: with grad enabled the stepper hands out private copies of what a step wrote (pack.grad_copies: four
small copy launches per step), which is what keeps an episode's backward() correct; under no_grad it hands out its own
buffers.  An episode is begin + n steps on a recorded tour (no policy ops); a figure is the median of ``--calls``
synchronised episodes (scripts/time_policy_head.py's timing loop) divided by n, taken in two runs with the two modes
alternating.  ``host`` is the time to ISSUE the episode (no synchronise inside the bracket).  No speed bar.  Usage:

    python scripts/time_grad_step.py [--calls 200] [--warmup 10]
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
from time_policy_head import two_runs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, n = 8192, 10
    st, dy = synth.rand_instances(B, n, 2, seed=7)
    tape = synth.random_feasible_tape(st, dy, n, seed=8).to(dev).t().contiguous()      # (n, B): a step's picks are one row
    st, dy = st.to(dev), dy.to(dev)
    env = T.BatchedContainer(B, [5, 50], n, "C+P+S-lb-soft", "diff", device=dev)
    sp = T.EpisodeStepper(st, dy, env, steps=n)

    def episode():
        sp.begin(st, dy)
        for k in range(n):
            sp.step(tape[k])

    def under(mode):
        def run():
            with mode():
                episode()
        return run

    def host_us(mode):
        run = under(mode)
        ts = []
        for _ in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
        return round(statistics.median(ts[args.warmup:]) / n, 2)
    pack.set_binary_check('trust')
    try:
        res = two_runs({"no_grad": under(torch.no_grad), "grad_enabled": under(torch.enable_grad)}, args.calls, args.warmup)
        row = {"shape": "c2", "B": B, "n": n,
               "step_us": {k: [round(v / n, 2) for v in vs] for k, vs in res.items()},
               "host_us_per_step": {"no_grad": host_us(torch.no_grad), "grad_enabled": host_us(torch.enable_grad)}}
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    print(json.dumps(row))


if __name__ == "__main__":
    main()
