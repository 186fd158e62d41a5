#!/usr/bin/env python3
"""MACS / MUL whole episodes above 64 cells: the one-launch form (pack.episode_scores -> tap_episode_scores ->
k_macs2d_wave_episode / k_macs3d_wave_episode) against the stepped form (pack._stepped_scores: n eager placement launches on a
state blob, what episode_scores ran for these shapes before), same inputs, one process.

    python scripts/time_macs_wave_episode.py [--out profiles/macs_wave_episode.json] [--reps 25] [--runs 2]
    python scripts/time_macs_wave_episode.py --steps --label parent     (with TAP_LIB_PATH=<the parent commit's libtapenv.so>)
    python scripts/time_macs_wave_episode.py --steps --label change

Episodes: per shape and batch size the median wall time of --reps synchronised calls after three warm-up calls, the
whole measurement --runs times over (the spread between runs is the band a difference has to clear); the two forms'
results are compared bit for bit and the launch record must show the one-launch kernel.  --steps: eager microseconds
per placement step of the wave STEP kernels (k_macs2d_wave_step / k_macs3d_wave_step, which share the placement body
with the episode kernels), stored under --label: run it on the parent's library and on this one, twice each.  Results
are merged into --out: `method` / `episodes` and `step_kernels_us_per_eager_step` are this script's, any other section
of the file (the forced-build A/B of the 3D kernel's two register builds, made with libraries compiled for the purpose
and TAP_LIB_PATH) is kept as it is.  `register_tight_build` in a row: which of the two builds of k_macs3d_wave_episode
the launcher took (the launch record's mode field)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                          # noqa: E402
import tap_net_amd as T                               # noqa: E402
from tap_net_amd import _lib, pack                    # noqa: E402

DEV = "cuda:0"
REWARD = "C+P+S-mcs-soft"
SHAPES = [("macs2d_W100_n10", [100, 50], 10), ("macs3d_10x10_n10", [10, 10, 50], 10), ("macs3d_20x20_n30", [20, 20, 30], 30)]
BATCHES = (128, 4096)
STEP_CASES = [("macs2d_W100_n10_B4096", [100, 50], 10, 4096), ("macs3d_10x10_n10_B4096", [10, 10, 50], 10, 4096),
              ("macs3d_20x20_n30_B1024", [20, 20, 30], 30, 1024)]


def _inputs(cs, n, B):
    """static in PACKDataset's layout without rotations (B, 1 + D, n) and one random tour per container"""
    D = len(cs)
    rng = np.random.RandomState(1)
    blocks = rng.randint(1, 5, size=(B, n, D)).astype(np.float32)
    static = torch.zeros(B, 1 + D, n, device=DEV)
    static[:, 0] = torch.arange(n, device=DEV)
    static[:, 1:] = torch.as_tensor(blocks, device=DEV).transpose(1, 2)
    tour = torch.as_tensor(np.stack([rng.permutation(n) for _ in range(B)]), device=DEV, dtype=torch.int64)
    return static.contiguous(), tour.contiguous()


def _median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def episodes(reps, runs):
    out = []
    for run in range(runs):
        for name, cs, n in SHAPES:
            for B in BATCHES:
                static, tour = _inputs(cs, n, B)
                one = lambda: pack.episode_scores(static, tour, REWARD, "bot", False, cs, "MACS", check=False)     # noqa: E731
                stepped = lambda: pack._stepped_scores(static, tour, cs, n, REWARD, "MACS", None, check=False)      # noqa: E731
                _lib.variant_hits_reset(DEV)
                r1, s1 = one()
                kind = _lib.TAP_HIT_EPISODE_MACS2_WAVE if len(cs) == 2 else _lib.TAP_HIT_EPISODE_MACS3_WAVE
                hit = [k for k in _lib.variant_hits(DEV) if k[0] == kind]
                assert len(hit) == 1, "episode_scores did not take the one-launch kernel for %s" % name
                r2, s2 = stepped()
                same = bool(((r1 == r2) | (torch.isnan(r1) & torch.isnan(r2))).all()) and torch.equal(s1, s2)
                assert same, "one-launch and stepped results differ for %s B=%d" % (name, B)
                t_one, t_step = _median_ms(one, reps), _median_ms(stepped, reps)
                row = dict(run=run, shape=name, container=cs, n=n, B=B, waves_per_workgroup=hit[0][5], register_tight_build=hit[0][4],
                           one_launch_ms=round(t_one, 4),
                           stepped_ms=round(t_step, 4), stepped_over_one_launch=round(t_step / t_one, 3),
                           flagged=int(torch.isnan(r1).sum().item()))
                print(json.dumps(row), flush=True)
                out.append(row)
    return out


def steps(reps):
    out = []
    for name, cs, n, B in STEP_CASES:
        rng = np.random.RandomState(1)
        blocks = torch.as_tensor(rng.randint(1, 5, size=(B, n, len(cs))).astype(np.int32), device=DEV)
        cols = [blocks[:, t].contiguous() for t in range(n)]
        env = T.BatchedContainer(B, cs, n, REWARD, "diff", packing_strategy="MACS", device=DEV)
        ts = []
        for rep in range(reps + 2):
            env.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(n):
                env.add_new_blocks(cols[t])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / n * 1e6)
        row = dict(case=name, us_per_eager_step=round(statistics.median(ts[2:]), 2), min_us=round(min(ts[2:]), 2))
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "macs_wave_episode.json"))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--label", default="change")
    a = ap.parse_args()
    assert a.reps >= 20 or a.steps, "the episode figures are medians of at least 20 calls"
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["device"] = torch.cuda.get_device_name(0)
    if a.steps:
        doc.setdefault("step_kernels_us_per_eager_step", {}).setdefault(a.label, []).append(steps(max(a.reps, 7)))
    else:
        doc["method"] = "median wall ms of %d synchronised calls after 3 warm-up calls, %d runs; check=False on both forms" % (a.reps, a.runs)
        doc["episodes"] = episodes(a.reps, a.runs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
