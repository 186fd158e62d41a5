#!/usr/bin/env python3
"""Time the dynamic encoder on the bit shadow (encode.hip: tap_encode_bits, one launch) against the capturable torch
form of the same line of the loop (model.py:380) as the code ran before it: the fp32 ``dynamic`` the step writes, then
``F.conv1d`` on it.  B = 8 192, H = 128, windows (rows, nR) = (30, 20) [c2], (30, 60) [c3], (126, 84):

  encode_bits        the new launch on kept buffers (with a bias), on the instances' own shadow (about 9 % ones)
  encode_bits_ones   the same on an all-ones shadow: the sparse kernel's worst case (one addition per row)
  conv1d             F.conv1d on an fp32 0/1 tensor of the window's shape, alone
  expansion          what the step pays to write that tensor: a policy-free episode (a replayed tour) on
                     EpisodeStepper(expand_dynamic=True) minus the same on expand_dynamic=False, per step (c2 and c3;
                     not measured at (126, 84), whose 42-step episode is not part of this script)
  backward           tap_encode_bits_backward (two launches) against torch's conv1d weight / bias gradients
  store_ceiling      scripts/calibrate_bw.py's fill of out's bytes (plain and nontemporal 16-byte stores, the better one)

and one episode-level pair at c2, ten steps from a hipGraph: expand_dynamic=False + the encoder + a fixed linear scorer
(v . tanh(hidden)) + pointer_pick, against expand_dynamic=True + F.conv1d + the same rest.

Clock: device events around a replay of a hipGraph holding ``--per-graph`` calls (one episode for the episode rows),
after warm-ups; every figure is the median of ``--reps`` replays, the two sides alternating, two runs each.  No speed
bar: the numbers are recorded as they come out.  Writes profiles/dyn_encoder.json, rewritten after every row.  Usage:

    python scripts/time_dyn_encoder.py [--reps 30] [--per-graph 8] [--out profiles/dyn_encoder.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tap_net_amd as T  # noqa: E402
from tap_net_amd import _lib, pack, rollout, synth  # noqa: E402

B, H = 8192, 128
# rows = 3 n, nR = n * R; the container is the one the expansion's share is measured on (None: the call-level rows only)
WINDOWS = [("c2", 2, 10, [5, 50]), ("c3", 3, 10, [5, 5, 50]), ("n42", 2, 42, None)]


def captured(fn, dev, times=1):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(times):
            keep = fn()
    return graph, keep


def replay_us(graph, reps, per):
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / per)
    return statistics.median(ts)


def two_runs(graphs, reps, per):
    out = {k: [] for k in graphs}
    for _ in range(2):
        for k, g in graphs.items():
            out[k].append(round(replay_us(g, reps, per), 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--per-graph", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dyn_encoder.json"))
    args = ap.parse_args()
    import calibrate_bw
    dev = torch.device("cuda", 0)
    per = args.per_graph
    rows_out = []

    def write(episode=None):
        """the file as it stands: rewritten after every row, so a run that is cut short leaves the rows it measured
        (``episode`` null until the episode pair has been measured)"""
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev),
                       "note": "device events around hipGraph replays (%d calls per graph, one episode for the step / episode rows), "
                               "medians of %d replays after warm-ups, two runs each, sides alternating; store ceiling = "
                               "calibrate_bw.run fill / fill_nt of out's bytes, warm" % (per, args.reps),
                       "rows": rows_out, "episode": episode}, f, indent=1)

    pack.set_binary_check('trust')
    try:
        for name, D, n, cs in WINDOWS:
            st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
            rows, nR = int(dy.shape[1]), int(dy.shape[2])
            bits = pack.dynamic_bits(dy)[0]
            enc = T.DynamicBitsEncoder(rows, H).to(dev)
            W, bias = enc.conv.weight.detach(), enc.conv.bias.detach()
            W2 = W.squeeze(2).contiguous()
            out = torch.empty(B, H, nR, device=dev)
            out_bytes = out.numel() * 4
            with torch.no_grad():
                f_enc = lambda: rollout._encode_into(bits, W2, bias, rows, out)              # noqa: E731
                f_conv = lambda: F.conv1d(dy, W, bias)                                       # noqa: E731
                assert torch.allclose(rollout.encode_dynamic_bits(bits, W, bias), f_conv(), atol=1e-4)
                ones = torch.full_like(bits, -1)
                f_ones = lambda: rollout._encode_into(ones, W2, bias, rows, out)             # noqa: E731
                graphs = {"encode_bits": captured(f_enc, dev, per)[0], "conv1d": captured(f_conv, dev, per)[0],
                          "encode_bits_ones": captured(f_ones, dev, per)[0]}
                res = two_runs(graphs, args.reps, per)
                # the expansion's share of a step: a replayed tour on the two stepper forms
                steps, expansion = {}, None
                if cs is not None:
                    tape = torch.arange(n, device=dev).repeat(B, 1)                 # any tour: the step's cost does not depend on it
                    ep_graphs = {}
                    for label, expand in (("step_lean", False), ("step_expanded", True)):
                        env = T.BatchedContainer(B, cs, n, "C+P+S-lb-soft", "diff", device=dev)
                        sp = T.EpisodeStepper(st, dy, env, 'bot', True, steps=n, expand_dynamic=expand)
                        pol = T.TapePolicy(tape)
                        ep = lambda sp=sp, pol=pol: T.run_episode(st, dy, pol, cs[0], cs[-1], stepper=sp, check=False)["reward"]   # noqa: E731
                        ep_graphs[label] = captured(ep, dev)[0]
                    steps = two_runs(ep_graphs, args.reps, n)
                    expansion = [round(a - b, 2) for a, b in zip(steps["step_expanded"], steps["step_lean"])]
            # the backward against torch's
            g = torch.randn(B, H, nR, device=dev)
            L, c = _lib.lib(), _lib.ctx(dev)
            need = int(L.tap_encode_bits_backward_scratch(B, nR, rows, H))
            scratch = torch.empty(need // 4, device=dev)
            dW, db = torch.empty(H, rows, device=dev), torch.empty(H, device=dev)
            f_bw = lambda: _lib.check(L.tap_encode_bits_backward(c, _lib.ptr(bits), _lib.ptr(g), B, nR, rows, H, _lib.ptr(dW),   # noqa: E731
                                                                 _lib.ptr(db), _lib.ptr(scratch), need, _lib.stream_of(dev)), c)
            f_tbw = lambda: (torch.einsum('bhc,brc->hr', g, dy), g.sum((0, 2)))              # noqa: E731
            with torch.no_grad():
                bw = two_runs({"backward": captured(f_bw, dev, per)[0], "torch_backward": captured(f_tbw, dev, per)[0]}, args.reps, per)
            ceil = max(calibrate_bw.run(k, out_bytes, False, dev)["GBps"] for k in (2, 3))
            row = {"window": name, "B": B, "H": H, "rows": rows, "nR": nR, "out_bytes": out_bytes, "dynamic_fp32_bytes": B * rows * nR * 4,
                   "shadow_bytes": bits.numel() * 8, "ones_share": round(float(dy.mean().item()), 4), "store_ceiling_GBps": ceil, "store_ceiling_us": round(out_bytes / ceil / 1e3, 2),
                   "expansion_us_per_step": expansion, "scratch_bytes": need}
            row.update({k + "_us": v for k, v in list(res.items()) + list(steps.items()) + list(bw.items())})
            row["conv1d_plus_expansion_us"] = None if expansion is None else [round(a + b, 2) for a, b in zip(res["conv1d"], expansion)]
            row["encode_bits_fraction_of_store_ceiling"] = [round(out_bytes / ceil / 1e3 / t, 3) for t in res["encode_bits"]]
            row["conv1d_fraction_of_store_ceiling"] = [round(out_bytes / ceil / 1e3 / t, 3) for t in res["conv1d"]]
            rows_out.append(row)
            print(json.dumps(row), flush=True)
            write()
        # the ten-step c2 episode from a hipGraph: lean + encoder against expanded + conv1d, the same scorer and head
        name, D, n, cs = WINDOWS[0]
        st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
        enc = T.DynamicBitsEncoder(3 * n, H).to(dev)
        v = torch.randn(H, device=dev)
        graphs, keeps = {}, {}
        with torch.no_grad():
            for label, lean in (("lean_encoder", True), ("expanded_conv1d", False)):
                env = T.BatchedContainer(B, cs, n, "C+P+S-lb-soft", "diff", device=dev)
                sp = T.EpisodeStepper(st, dy, env, 'bot', True, steps=n, expand_dynamic=not lean)
                src = (lambda sp=sp: sp.dynamic_bits) if lean else (lambda sp=sp: sp.dynamic)
                scorer = lambda src=src, **_: (torch.tanh(enc(src())) * v[None, :, None]).sum(1)                       # noqa: E731
                pol = T.PointerHeadPolicy(scorer, greedy=True)

                def ep(sp=sp, pol=pol):
                    out = T.run_episode(st, dy, pol, cs[0], cs[-1], stepper=sp, check=False)
                    return out["tour_idx"], out["reward"], pol.tour_logp()
                graphs[label], keeps[label] = captured(ep, dev)
            res = two_runs(graphs, args.reps, 1)
        same = float((keeps["lean_encoder"][0] == keeps["expanded_conv1d"][0]).float().mean().item())
        episode = {"window": "c2", "B": B, "H": H, "steps": n, "scorer": "v . tanh(hidden)", "picks_equal": round(same, 5)}
        episode.update({k + "_episode_us": t for k, t in res.items()})
        print(json.dumps(episode), flush=True)
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    write(episode)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
