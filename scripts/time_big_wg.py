#!/usr/bin/env python3
"""Eager and graph-replayed microseconds per decoding step on the one-workgroup-per-container LB_GREEDY kernels
(big.hip: k_big_wg_step, containers of 4 097 .. 16 384 cells): 3D 100 x 100 x 60 and 128 x 128 x 60, 2D 8 192 x 100,
soft and hard rewards, B = 256 / 1 024 / 4 096.  One step = BatchedContainer.add_new_blocks with its 'diff' feature.

    python scripts/time_big_wg.py [--threads 256|512|1024] [--batches 256,1024,4096] [--out rows.jsonl]

--threads sets TAP_BIG_WG_THREADS (threads per container) for this process.  Only a library built with -DTAP_AB_BUILD
reads that variable (tap_common.h: tap_ab_env): point TAP_LIB_PATH at one (a copy of tap-net_amd/csrc built with
-DTAP_AB_BUILD behind the Makefile's CXXFLAGS, given whole in the environment); on a library that ignores the variable --threads is refused, so no row gets a label it did not run
with.  Blocks: 3D sides 4 .. 16 (the wide stability path above 8), 2D widths 100 .. 999, heights 1 .. 4 (no overflow
within the episode)."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--threads", type=int, default=0)
ap.add_argument("--batches", default="256,1024,4096")
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--out", default="")
ap.add_argument("--shapes", default="all")
args = ap.parse_args()
if args.threads:
    os.environ["TAP_BIG_WG_THREADS"] = str(args.threads)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                    # noqa: E402
import torch                          # noqa: E402
import tap_net_amd as T               # noqa: E402
if args.threads and b"TAP_BIG_WG_THREADS" not in open(T._lib.LIB_PATH, "rb").read():   # the name is only in a library that reads it
    sys.exit("--threads: %s ignores TAP_BIG_WG_THREADS; set TAP_LIB_PATH to a -DTAP_AB_BUILD library" % T._lib.LIB_PATH)
DEV = "cuda:0"
assert torch.cuda.is_available(), "needs a GPU"
SHAPES = [([100, 100, 60], (4, 17)), ([128, 128, 60], (4, 17)), ([8192, 100], (100, 1000))]
if args.shapes != "all":
    SHAPES = [SHAPES[int(i)] for i in args.shapes.split(",")]


def blocks_for(cs, lo, hi, B, n):
    rs = np.random.RandomState(1)
    b = rs.randint(lo, hi, size=(B, n, len(cs))).astype(np.int32)
    b[:, :, -1] = rs.randint(1, 5, size=(B, n))
    return torch.as_tensor(b, device=DEV)


def eager(env, blocks, n):
    env.reset(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for t in range(n):
        env.add_new_blocks(blocks[:, t])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def replayed(env, blocks, n):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager(env, blocks, n)                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.reset()
        for t in range(n):
            env.add_new_blocks(blocks[:, t])
    g.replay(); torch.cuda.synchronize()
    reps = 3
    t0 = time.perf_counter()
    for _ in range(reps):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (reps * n) * 1e6      # (the reset launch included, one per n steps)


rows = []
n = args.steps
for cs, (lo, hi) in SHAPES:
    for reward in ("C+P+S-lb-soft", "C+P+S-lb-hard"):
        for B in [int(b) for b in args.batches.split(",")]:
            bl = [blocks_for(cs, lo, hi, B, n)[:, t].contiguous() for t in range(n)]
            blocks = torch.stack(bl, 1)
            env = T.BatchedContainer(B, cs, n, reward, "diff", device=DEV)
            blk = [b for b in bl]
            eager(env, torch.stack(blk, 1), n)                  # warm-up
            e = min(eager(env, blocks, n) for _ in range(2))
            env.check()
            try:
                r = replayed(env, blocks, n)
            except Exception as ex:                             # report, do not hide
                r = None
                print("graph capture failed:", repr(ex)[:200], flush=True)
            row = dict(shape="x".join(map(str, cs)), reward=reward, B=B, threads=int(os.environ.get("TAP_BIG_WG_THREADS", 0)) or "default",
                       eager_us_per_step=round(e, 1), replayed_us_per_step=None if r is None else round(r, 1), steps=n)
            rows.append(row)
            print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
