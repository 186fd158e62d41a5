#!/usr/bin/env python3
"""Time the decoding head (policy.hip: tap_policy_pick, one launch) against what a trainer writes in torch for the same
line of the loop (model.py:359-372), at B = 8 192 with nR = 20 (c2), nR = 60 (c3) and nR = 120, on randn * 3 logits and
masks of c2's live share (13 %, at least one column per row):

  head               pointer_pick's launch on buffers kept by the caller (sample, no probs; also greedy, and sample
                     with probs_out as the autograd path runs it)
  torch_reference    softmax(logits + mask.log()), Categorical(probs).sample(), log_prob -- the reference's expression
                     without its host loop; eager only (its multinomial is not capturable on this stack)
  torch_cumsum       the capturable form: softmax, cumsum against a pre-drawn u, argmax -- UniformPickPolicy's device
                     -- plus a log_softmax gather for logp; eager and replayed from a hipGraph

and one episode-level row: run_episode at c2 (2D, W = 5, n = 10) captured in a hipGraph with ONE fixed toy scorer (a
single matmul on decoder_dynamic), torch_cumsum as the head against PointerHeadPolicy.  Every figure is the median of
``--calls`` synchronised calls (host clock around the call and a device synchronise) after ``--warmup`` warm-ups, taken
in two runs, the two sides alternating.  No speed bar: the numbers are recorded as they come out.  Prints one line per
row and writes profiles/policy_head.json.  Usage:

    python scripts/time_policy_head.py [--calls 200] [--warmup 10] [--out profiles/policy_head.json]
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
from tap_net_amd import pack, rollout, synth  # noqa: E402

SHAPES = [("c2", 20), ("c3", 60), ("wide", 120)]
B = 8192


def median_us(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def two_runs(fns, calls, warmup):
    """{name: [run 1, run 2]} with the sides alternating inside each run"""
    out = {k: [] for k in fns}
    for _ in range(2):
        for k, fn in fns.items():
            out[k].append(round(median_us(fn, calls, warmup), 1))
    return out


def captured(fn, dev):
    """fn captured in a hipGraph after a warm-up on a side stream -> the graph"""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    return graph, keep


def torch_reference(logits, mask):
    probs = torch.softmax(logits + mask.log(), dim=1)              # model.py:359
    m = torch.distributions.Categorical(probs)                     # model.py:365-369, without the rejection loop
    ptr = m.sample()
    return ptr, m.log_prob(ptr)


def torch_cumsum(logits, mask, u):
    z = logits + mask.log()
    probs = torch.softmax(z, dim=1)
    ptr = (probs.cumsum(1) > u.unsqueeze(1)).to(torch.float32).argmax(1)
    return ptr, torch.log_softmax(z, dim=1).gather(1, ptr.unsqueeze(1)).squeeze(1)


class TorchHeadPolicy(object):
    """torch_cumsum as a policy: the same scorer, u and kept log-probabilities as PointerHeadPolicy"""

    def __init__(self, scorer, u):
        self.scorer, self.u, self.logp = scorer, u, []

    def __call__(self, step, current_mask, **kw):
        if step == 0:
            self.logp = []
        ptr, logp = torch_cumsum(self.scorer(step=step, current_mask=current_mask, **kw), current_mask, self.u[step])
        self.logp.append(logp)
        return ptr

    def tour_logp(self):
        return torch.stack(self.logp, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_head.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    rows = []
    with torch.no_grad():
        for name, nR in SHAPES:
            logits = torch.randn(B, nR, device=dev, generator=gen) * 3
            mask = (torch.rand(B, nR, device=dev, generator=gen) < 0.13).to(torch.float32)
            mask[torch.arange(B, device=dev), torch.randint(nR, (B,), device=dev, generator=gen)] = 1
            u = torch.rand(B, device=dev, generator=gen)
            ptr = torch.empty(B, dtype=torch.int64, device=dev)
            logp = torch.empty(B, dtype=torch.float32, device=dev)
            probs = torch.empty(B, nR, dtype=torch.float32, device=dev)
            head = lambda: rollout._pick_into(logits, mask, u, ptr, logp, None)                 # noqa: E731
            head_probs = lambda: rollout._pick_into(logits, mask, u, ptr, logp, probs)          # noqa: E731
            head_greedy = lambda: rollout._pick_into(logits, mask, None, ptr, logp, None)       # noqa: E731
            cums = lambda: torch_cumsum(logits, mask, u)                                        # noqa: E731
            # the two heads agree on these inputs wherever u * S is clear of a prefix sum (fp32 cumsum on torch's side)
            head()
            agree = float((ptr == cums()[0]).float().mean().item())
            g_head, _ = captured(head, dev)
            g_cums, _ = captured(cums, dev)
            res = two_runs({"head": head, "head_probs": head_probs, "head_greedy": head_greedy,
                            "torch_reference": lambda: torch_reference(logits, mask), "torch_cumsum": cums,
                            "head_graph": g_head.replay, "torch_cumsum_graph": g_cums.replay}, args.calls, args.warmup)
            row = {"shape": name, "B": B, "nR": nR, "live_columns_mean": round(float(mask.sum(1).mean().item()), 2),
                   "picks_equal_torch_cumsum": round(agree, 5)}
            row.update({k + "_us": v for k, v in res.items()})
            rows.append(row)
            print(json.dumps(row), flush=True)
        # one episode at c2 from a hipGraph: the same toy scorer under both heads
        n, Be = 10, B
        st, dy = synth.device_rand_instances(Be, n, 2, seed=7, device=dev)
        Wm = torch.randn(4, 2 * n, device=dev, generator=gen) * 0.05
        scorer = lambda decoder_dynamic, **_: decoder_dynamic.view(Be, 4) @ Wm                  # noqa: E731
        ue = torch.rand(n, Be, device=dev, generator=gen)
        episode = {}
        pack.set_binary_check('trust')
        try:
            graphs = {}
            for label, pol in (("torch_cumsum", TorchHeadPolicy(scorer, ue)), ("head", T.PointerHeadPolicy(scorer, u=ue))):
                env = T.BatchedContainer(Be, [5, 50], n, "C+P+S-lb-soft", "diff", device=dev)

                def ep(pol=pol, env=env):
                    out = T.run_episode(st, dy.clone(), pol, 5, 50, env=env)
                    return out["tour_idx"], out["reward"], pol.tour_logp()
                graphs[label] = captured(ep, dev)
            res = two_runs({k + "_episode_graph": g.replay for k, (g, _) in graphs.items()}, args.episodes, 3)
            same = float((graphs["head"][1][0] == graphs["torch_cumsum"][1][0]).float().mean().item())
            episode = {"shape": "c2", "B": Be, "n": n, "steps": n, "scorer": "decoder_dynamic (B, 4) @ (4, 20)",
                       "picks_equal": round(same, 5)}
            episode.update({k + "_us": v for k, v in res.items()})
            print(json.dumps(episode), flush=True)
            pack.check_binary()
        finally:
            pack.set_binary_check('check')
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev),
                   "note": "medians of %d synchronised calls (episodes: %d) after warm-ups, two runs each, sides alternating; "
                           "head = tap_policy_pick on kept buffers; torch_reference = softmax + Categorical.sample + log_prob "
                           "(eager only); torch_cumsum = softmax, cumsum > u, argmax + log_softmax gather" % (args.calls, args.episodes),
                   "rows": rows, "episode": episode}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
