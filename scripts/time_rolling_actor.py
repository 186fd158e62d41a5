#!/usr/bin/env python3
"""Time the fused pointer launch (pointer.hip: tap_pointer_pick_static, scores and pick in one launch) against the composition
it replaces, and the rolling actor module with ``fused_pick`` on against off.

  (a) one decoding step's pointer side from a hipGraph, under device events: ``fused`` = tap_pointer_pick_static on the
      ``static[:, 1:, :]`` view of a (B, 1 + S, nR) window, against ``composed`` = the copy of that view to contiguous memory,
      tap_pointer_scores_static and tap_policy_pick (greedy) -- what a step of the rolling loop runs without the fused
      launch.  c5's window (nR 20, rows 30, S 2) at Hd 128 and 256, each at B = 8 192 and B = 128.  A graph holds ``--reps``
      repetitions; a figure is one replay's device time divided by the repetitions.
  (b) the eval episode through ``tools.RollingDRL`` (eager, device events around the call): N = 50 blocks, windows of 10, 2D,
      He = Hd = 128, B = 8 192 and B = 128, ``fused_pick`` on against off -- two modules with the same weights, each with its own
      steppers; their tours are compared.

  (c) for orientation only, ``--reference-only COUNT``, without a GPU and only where the reference checkout is present: the
      reference's own rolling.DRL in rolling.validate's loop at (b)'s shape, batch 1, one CPU thread, per instance; the row is
      added to the file (a) and (b) wrote.

(a) and (b): both sides are this library in one process, the sides alternating inside every run; a figure is the median of
``--runs`` runs and its spread is max - min of that side's runs.  Prints one line per row and writes
profiles/rolling_actor.json.  Usage:

    python scripts/time_rolling_actor.py [--runs 7] [--reps 20] [--out profiles/rolling_actor.json]
    python scripts/time_rolling_actor.py --reference-only 3
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tap_net_amd as T  # noqa: E402
from tap_net_amd import generate as gen  # noqa: E402
from tap_net_amd import pack, rollout  # noqa: E402

NR, ROWS, S = 20, 30, 2
LAUNCH_SHAPES = [(Hd, B) for Hd in (128, 256) for B in (8192, 128)]
EPISODE = dict(N=50, child=10, D=2, init=[7, 250], height=260, He=128, Hd=128)


def captured(fn, dev, reps):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    return graph


def event_us(fn, per=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / per


def interleaved(sides, runs, per=1, warm=2):
    """{name: dict(median_us, spread_us, runs_us)}: the sides alternate inside every run"""
    for _ in range(warm):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in sides}
    for _ in range(runs):
        for k, fn in sides.items():
            ts[k].append(event_us(fn, per))
    return {k: dict(median_us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2), runs_us=[round(x, 2) for x in v])
            for k, v in ts.items()}


def verdict(res, a="fused", b="composed"):
    gain = res[b]["median_us"] - res[a]["median_us"]
    spread = max(res[a]["spread_us"], res[b]["spread_us"])
    return dict(gain_us=round(gain, 2), larger_spread_us=spread, gain_exceeds_spread=bool(gain > spread))


def launch_rows(dev, runs, reps):
    rows = []
    g = torch.Generator(device=dev).manual_seed(5)
    for Hd, B in LAUNCH_SHAPES:
        r = lambda *s: torch.randn(*s, device=dev, generator=g)                                # noqa: E731
        window = torch.randint(1, 6, (B, 1 + S, NR), device=dev, generator=g).float()
        view = window[:, 1:, :]
        bits = torch.randint(0, 1 << ROWS, (B, NR), device=dev, generator=g, dtype=torch.int64)
        G, gg, M, k, q = r(3 * Hd, S) * 0.1, r(3 * Hd) * 0.1, r(3 * Hd, ROWS) * 0.1, r(3 * Hd) * 0.1, r(B, Hd) * 0.5
        va, vp = r(Hd), r(Hd)
        mask = (torch.rand(B, NR, device=dev, generator=g) < 0.3).float()
        mask[torch.arange(B, device=dev), torch.randint(NR, (B,), device=dev, generator=g)] = 1
        ptr, logp = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, device=dev)
        ptr2, logp2 = torch.empty_like(ptr), torch.empty_like(logp)
        xs, logits, attn, t = torch.empty(B, S, NR, device=dev), torch.empty(B, NR, device=dev), torch.empty(B, NR, device=dev), torch.empty(B, Hd, device=dev)
        stride = rollout._rows_view_stride(view)

        def fused():
            rollout._pick_static_into(view, stride, bits, G, gg, M, k, q, va, vp, mask, None, ROWS, ptr, logp, None)

        def composed():
            xs.copy_(view)
            rollout._scores_static_into(xs, bits, G, gg, M, k, q, va, vp, ROWS, logits, attn, t)
            rollout._pick_into(logits, mask, None, ptr2, logp2, None)
        fused(), composed()
        torch.cuda.synchronize()
        same = bool(torch.equal(ptr, ptr2) and torch.equal(logp.view(torch.int32), logp2.view(torch.int32)))
        graphs = {"fused": captured(fused, dev, reps), "composed": captured(composed, dev, reps)}
        res = interleaved({name: gr.replay for name, gr in graphs.items()}, runs, per=reps)
        row = dict(kind="launch", B=B, nR=NR, rows=ROWS, S=S, Hd=Hd, reps_per_graph=reps, same_bytes=same, **res, **verdict(res))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def episode_rows(dev, runs):
    rows = []
    e = EPISODE
    for B in (8192, 128):
        _, _, blocks, positions = gen.generate_instances(B, e["N"], e["D"], e["init"][0], e["init"][-1], 1, (1, 5), seed=21, device=dev,
                                                         return_aux=True)
        torch.manual_seed(9)
        mods = {}
        for name, on in (("fused", True), ("composed", False)):
            m = T.RollingDRL(e["D"], 3 * e["child"], e["He"], e["Hd"], True, 'bot', True, 5, e["height"], e["D"], "C+P+S-lb-soft",
                             'shape_heightmap', "diff", "LB_GREEDY", None, None, None, fused_pick=on).to(dev).eval()
            if mods:
                m.load_state_dict(mods["fused"].state_dict(), strict=True)
            mods[name] = m
        out = {}

        def run(name):
            out[name] = mods[name](T.RollingWindows(blocks, positions, e["init"], e["child"]))
        res = interleaved({name: (lambda name=name: run(name)) for name in mods}, runs, warm=1)
        same = all(torch.equal(a.view(torch.int32) if a.dtype is torch.float32 else a, b.view(torch.int32) if b.dtype is torch.float32 else b)
                   for a, b in zip(out["fused"], out["composed"]))
        row = dict(kind="episode", B=B, N=e["N"], child=e["child"], D=e["D"], He=e["He"], Hd=e["Hd"], mode="eval, eager", same_bytes=bool(same),
                   reward_nan=int(torch.isnan(out["fused"][3]).sum()), **res, **verdict(res))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def reference_row(count):
    """(c) the reference's own rolling.validate loop (rolling.py:579-637) per instance on this host's CPU, one thread, float32,
    the episode rows' shape with freshly initialised weights -> a row, or None where the reference checkout is absent"""
    import time

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_loader
    mods = ref_loader.load()
    if mods is None:
        return None
    tools, rpack, generate = mods
    sys.path.insert(0, ref_loader.REFERENCE_DIR)
    try:
        import rolling
    finally:
        sys.path.remove(ref_loader.REFERENCE_DIR)
    e = EPISODE
    torch.set_num_threads(1)
    torch.manual_seed(9)
    container = tools.Container([5, e["height"]], e["N"], "C+P+S-lb-soft", "diff", packing_strategy="LB_GREEDY")
    actor = rolling.DRL(e["D"], 3 * e["child"], e["He"], e["Hd"], False, "bot", True, 5, e["height"], e["D"], "C+P+S-lb-soft",
                        "shape_heightmap", "diff", "LB_GREEDY", [container], rpack.update_dynamic, rpack.update_mask, 1, 0.1, 1).eval()
    ts = []
    for i in range(count):
        np.random.seed(300 + i)
        rot, pos, _, _, _ = generate.generate_blocks(e["N"], list(e["init"]), 1, [1, 5])
        blocks = np.asarray(rot).reshape(2, e["D"], e["N"]).transpose(0, 2, 1).reshape(2 * e["N"], e["D"])
        ic = generate.InitialContainer(blocks, np.asarray(pos).reshape(e["D"], e["N"]).T, e["N"], list(e["init"]), True, e["child"], "bot")
        t0 = time.perf_counter()
        with torch.no_grad():
            one_step, last_hh = True, None
            ds, dd = torch.zeros(1, e["D"], 1), torch.zeros(1, 4, 1)
            while one_step:
                static, dynamic = ic.convert_to_input()
                static, dynamic = torch.FloatTensor(static).unsqueeze(0), torch.FloatTensor(dynamic).unsqueeze(0)
                if ic.is_last_graph():
                    one_step = False
                ptr, (ds, dd), last_hh = actor(static, dynamic, [ds, dd], last_hh, one_step)
                ic.remove_block(ic.sub_graph_nodes[int(ptr.numpy()[0]) % e["child"]])
        ts.append(time.perf_counter() - t0)
        container.clear_container()
    return dict(kind="reference_cpu", what="rolling.DRL in rolling.validate's loop, batch 1, one CPU thread, float32", N=e["N"],
                child=e["child"], D=e["D"], He=e["He"], Hd=e["Hd"], instances=count, ms_per_instance=[round(t * 1e3, 1) for t in ts],
                median_ms_per_instance=round(statistics.median(ts) * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_actor.json"))
    ap.add_argument("--reference-only", type=int, default=0, metavar="COUNT",
                    help="no GPU: time the reference's loop on COUNT instances on this CPU and add the row to --out")
    args = ap.parse_args()
    if args.reference_only:
        row = reference_row(args.reference_only)
        if row is None:
            sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
        print(json.dumps(row), flush=True)
        with open(args.out) as f:
            doc = json.load(f)
        doc["reference_cpu"] = row
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
        print("added reference_cpu to", args.out)
        return
    dev = torch.device("cuda", 0)
    pack.set_binary_check('trust')
    try:
        with torch.no_grad():
            rows = launch_rows(dev, args.runs, args.reps) + episode_rows(dev, args.runs)
    finally:
        pack.set_binary_check('check')
    keep = any(r["gain_exceeds_spread"] for r in rows)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev),
                   "note": "device events; medians of %d runs, the sides alternating inside every run; spread = max - min of a side's "
                           "runs; launch rows: one graph replay of %d repetitions, divided by the repetitions; fused = "
                           "tap_pointer_pick_static on the strided view; composed = copy of the view + tap_pointer_scores_static + "
                           "tap_policy_pick (greedy); episode rows: RollingDRL.forward eager, fused_pick on / off" % (args.runs, args.reps),
                   "fused_pick_default_justified": bool(keep), "rows": rows}, f, indent=1)
    print("wrote", args.out, "fused_pick default justified:", keep)


if __name__ == "__main__":
    main()
