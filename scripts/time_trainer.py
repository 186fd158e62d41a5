#!/usr/bin/env python3
"""Time the tail of a training iteration -- tap_net_amd.trainer's three launches (reinforce_seeds, ClipAdam.step) -- against
stock torch, and the whole iteration (TrainStep) eager and replayed from one graph.

  (a) tail     at the parameter sets of the Hd = 128 and Hd = 256 actors (He = 128) plus the H = 128 critic, B = 128, n = 10,
               random gradients.  This side: the three launches.  The other side: the reference's loss lines with their
               backward to tour_logp and critic_est, clip_grad_norm_ per module and Adam.step() per module, once with
               Adam(foreach=True) and once with Adam(fused=True, capturable=True).  Eager, and from a graph where the form can
               be captured (foreach Adam reads its step on the host: eager only).
  (b) iteration at c2's shape (2D, W = 5, n = 10, He = Hd = 128) with B = 128 and B = 8 192, dropout 0.1, free-running:
               TrainStep(tail='torch').step -- the hand-assembled loop --, TrainStep(tail='hip').step, and TrainStep.replay.

Device events around each call, one synchronisation per repetition; every figure is the median of ``--reps`` repetitions
after warm-ups; each side is measured ``--runs`` times after one discarded round, the sides alternating in an order that
reverses every round; spread = max - min of a side's runs.  Writes profiles/trainer.json, rewritten after every row.

    python scripts/time_trainer.py [--reps 20] [--runs 3] [--out profiles/trainer.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tap_net_amd as T  # noqa: E402
from tap_net_amd import pack, synth  # noqa: E402
from time_decoder_dropout import eager_us  # noqa: E402
from time_drl import alternate  # noqa: E402

N = 10


def modules(He, Hd, Hc, dev, dropout=0.1):
    actor = T.DRL(2, 3 * N, He, Hd, True, 'bot', True, 5, 50, 2, "C+P+S-lb-soft", 'shape_heightmap', 'diff', 'LB_GREEDY',
                  pack.update_dynamic, pack.update_mask, 1, dropout, seed=11).to(dev)
    critic = T.StateCritic(2, 3 * N, Hc).to(dev)
    for p in critic.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    return actor.train(), critic.train()


def captured(fn, dev):
    """fn after three warm-up calls on a side stream -> a graph's replay, or the exception's text"""
    try:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return graph.replay
    except Exception as e:                                       # noqa: BLE001 -- the row records what stopped the capture
        torch.cuda.synchronize(dev)
        return "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])


def summary(res):
    return {"median_us": {k: statistics.median(v) for k, v in res.items()}, "spread_us": {k: round(max(v) - min(v), 2) for k, v in res.items()}}


def tail_row(Hd, args, dev):
    B = 128
    mine, foreach, fused = (modules(128, Hd, 128, dev) for _ in range(3))
    reward, logp = -torch.rand(B, device=dev), -torch.rand(B, N, device=dev)
    est = torch.randn(B, device=dev)
    grads = [[torch.randn_like(p) * 0.01 for p in m.parameters()] for m in mine]
    row = {"actor_Hd": Hd, "B": B, "n": N, "actor_params": sum(p.numel() for p in mine[0].parameters()), "actor_tensors": len(grads[0]),
           "critic_params": sum(p.numel() for p in mine[1].parameters()), "critic_tensors": len(grads[1])}
    opt = T.ClipAdam([(list(m.parameters()), 5e-4, 2.0) for m in mine], zero_grads=False)
    row["chunks"] = opt.nchunks
    for m, gs in zip(mine, grads):
        for p, g in zip(m.parameters(), gs):
            p.grad.copy_(g)

    def ours():
        T.reinforce_seeds(reward, est, logp)
        opt.step()

    def torch_tail(mods, optims):
        e, lp = est.detach().requires_grad_(), logp.detach().requires_grad_()
        advantage = reward - e
        actor_loss = torch.mean(advantage.detach() * lp.sum(dim=1))
        critic_loss = torch.mean(advantage ** 2)
        torch.autograd.grad([actor_loss, critic_loss], [lp, e], [torch.ones_like(actor_loss), torch.ones_like(critic_loss)])
        for m, o in zip(mods, optims):
            torch.nn.utils.clip_grad_norm_(m.parameters(), 2.0)
            o.step()
    sides = {"three_launches": ours}
    for name, mods, kw in (("torch_foreach", foreach, dict(foreach=True)), ("torch_fused_capturable", fused, dict(fused=True, capturable=True))):
        for m, gs in zip(mods, grads):
            for p, g in zip(m.parameters(), gs):
                p.grad = g.clone()
        optims = [torch.optim.Adam(m.parameters(), lr=5e-4, **kw) for m in mods]
        sides[name] = (lambda mods=mods, optims=optims: torch_tail(mods, optims))
    res = alternate(sides, args.runs, lambda f: eager_us(f, args.reps))
    row["eager_us"], row["eager"] = res, summary(res)
    graphs = {"three_launches": captured(ours, dev), "torch_fused_capturable": captured(sides["torch_fused_capturable"], dev)}
    row["graph_capture_errors"] = {k: v for k, v in graphs.items() if isinstance(v, str)}
    graphs = {k: v for k, v in graphs.items() if not isinstance(v, str)}
    if graphs:
        res = alternate(graphs, args.runs, lambda f: eager_us(f, args.reps))
        row["graph_us"], row["graph"] = res, summary(res)
    return row


def iteration_row(B, args, dev, write, rows_out):
    st, dy = synth.device_rand_instances(B, N, 2, seed=7, device=dev)
    batch = (st, dy, torch.zeros(B, 2, 1, device=dev), torch.zeros(B, 4, 1, device=dev))
    row = {"shape": "c2", "B": B, "n": N, "He": 128, "Hd": 128, "critic_H": 128}
    rows_out.append(row)
    steps = {tail: T.TrainStep(*modules(128, 128, 128, dev), 5e-4, 5e-4, 2.0, 2, 'shape_heightmap', tail=tail) for tail in ('torch', 'hip')}
    sides = {"hand_assembled_torch_tail": lambda: steps['torch'].step(*batch), "train_step": lambda: steps['hip'].step(*batch)}
    res = alternate(sides, args.runs, lambda f: eager_us(f, args.reps))
    row["eager_us"], row["eager"] = res, summary(res)
    write()
    graph = T.TrainStep(*modules(128, 128, 128, dev), 5e-4, 5e-4, 2.0, 2, 'shape_heightmap', tail='hip')
    try:
        graph.capture(*batch)
    except Exception as e:                                       # noqa: BLE001
        torch.cuda.synchronize(dev)
        row["capture_error"] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:300])
        write()
        return
    sides = {"train_step": sides["train_step"], "replay": lambda: graph.replay(*batch)}
    res = alternate(sides, args.runs, lambda f: eager_us(f, args.reps))
    row["replay_us"], row["replay"] = res, summary(res)
    m, s = row["replay"]["median_us"], row["replay"]["spread_us"]
    row["replay_beats_step_by_more_than_spread"] = bool(m["train_step"] - m["replay"] > max(s.values()))
    write()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainer.json"))
    ap.add_argument("--only", default=None, choices=[None, "tail", "iteration"])
    args = ap.parse_args()
    if args.reps < 20 or args.runs < 3:
        raise SystemExit("at least 20 repetitions and 3 runs per side")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev),
           "note": "device events around each call, one synchronisation per repetition; medians of %d repetitions, %d runs per side after "
                   "one discarded round, sides alternating; spread = max - min of a side's runs; microseconds" % (args.reps, args.runs),
           "tail": [], "iteration": []}

    def write():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    pack.set_binary_check('trust')
    torch.manual_seed(3)
    try:
        if args.only in (None, "tail"):
            for Hd in (128, 256):
                out["tail"].append(tail_row(Hd, args, dev))
                write()
                print(json.dumps(out["tail"][-1]), flush=True)
        if args.only in (None, "iteration"):
            for B in (128, 8192):
                iteration_row(B, args, dev, write, out["iteration"])
                print(json.dumps(out["iteration"][-1]), flush=True)
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    write()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
