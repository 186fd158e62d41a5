#!/usr/bin/env python3
"""Time a TRAINING decoding step with the pointer's dropouts inside the decoder step's launch (tap_decoder_step_dropout /
tap_decoder_step_hm_dropout; tools.Pointer.forward_step_dropout) against what the same step costs without it: the torch
path that ``forward_step`` falls back to when dropout is active -- the decoder's convolutions, nn.GRU, two nn.Dropout, q and
the per-step M / k products (tools.Pointer.forward_bits).  p = 0.1 (the reference trainer's), training mode.

Shapes: the c2 step (Ks 2, Kd 4; rows 30, nR 20) at B = 8 192 with Hd = He = 128 and with the reference's default 256, and
the 3D step of profiles/heightmap_step.json (map 2 x 5 x 5, m 128, Hd 256, He 128, Ks 3; rows 30, nR 60; B = 4 096).

  (a) launch             the dropout launch against the plain launch on kept buffers: the generator's cost (hipGraph replays,
                         ``--per-graph`` calls per graph, device events)
  (b) step               forward, and forward + backward to every leaf, of one step: forward_step_dropout against
                         convolutions + forward_bits with torch's dropout
  (c) episode            the ten-step training episode on a lean stepper with the head (pointer_pick from pre-drawn u),
                         forward + backward to every parameter

(b) and (c) run eagerly, as a training loop does -- device events around the call, one synchronisation per repetition --, the
two sides alternating.  Every figure is the median of ``--reps`` repetitions; each side is measured ``--runs`` times and the
row keeps every run: the spread is max - min of a side's runs.  Writes profiles/decoder_dropout.json, rewritten after every
row.  Usage:

    python scripts/time_decoder_dropout.py [--reps 20] [--runs 3] [--per-graph 4] [--only SHAPE] [--out profiles/decoder_dropout.json]
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
from tap_net_amd import pack, rollout, synth  # noqa: E402
from time_dyn_encoder import captured, replay_us  # noqa: E402

P_DROP = 0.1
SHAPES = [dict(name="c2_Hd128", D=2, B=8192, He=128, Hd=128, cs=[5, 50], hm=None),
          dict(name="c2_Hd256", D=2, B=8192, He=256, Hd=256, cs=[5, 50], hm=None),
          dict(name="c3_heightmap_Hd256", D=3, B=4096, He=128, Hd=256, cs=[5, 5, 50], hm=(2, 5, 5, 128))]


def eager_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def alternate(sides, runs, clock):
    """{label: fn or graph} -> {label: [median of each run]}, the sides alternating within every run"""
    out = {k: [] for k in sides}
    for _ in range(runs):
        for k, s in sides.items():
            out[k].append(round(clock(s), 2))
    return out


def summary(res, ours, parent):
    """median and spread (max - min) of both sides' runs, the gain and whether it exceeds the larger spread"""
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: round(max(v) - min(v), 2) for k, v in res.items()}
    gain = med[parent] - med[ours]
    return {"median_us": med, "spread_us": spread, "gain_us": round(gain, 2), "factor": round(med[parent] / med[ours], 3),
            "gain_exceeds_larger_spread": bool(gain > max(spread.values()))}


def xavier(m):
    for p in m.parameters():
        torch.nn.init.xavier_uniform_(p) if p.dim() > 1 else torch.nn.init.normal_(p, std=0.1)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--per-graph", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_dropout.json"))
    ap.add_argument("--only", default=None, help="measure this shape alone and replace its row in --out, keeping the other rows")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    per, rows_out = args.per_graph, []
    shapes = [S for S in SHAPES if args.only in (None, S["name"])]
    if args.only:
        if not shapes:
            ap.error("--only takes one of %s" % ", ".join(S["name"] for S in SHAPES))
        with open(args.out) as f:
            rows_out = [r for r in json.load(f)["rows"] if r["shape"] != args.only]

    def write():
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "p": P_DROP,
                       "note": "(a): device events around hipGraph replays (%d launches per graph); (b), (c): device events around eager "
                               "calls, one synchronisation per repetition; medians of %d repetitions, %d runs per side, sides alternating; "
                               "spread = max - min of a side's runs; microseconds" % (per, args.reps, args.runs),
                       "rows": rows_out}, f, indent=1)
    pack.set_binary_check('trust')
    torch.manual_seed(3)
    try:
        for S in shapes:
            D, B, He, Hd, cs, n = S["D"], S["B"], S["He"], S["Hd"], S["cs"], 10
            net = xavier(T.Pointer(He, Hd, 'shape_heightmap', 'bot', dropout=P_DROP)).to(dev).train()
            st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
            rows, nR = int(dy.shape[1]), int(dy.shape[2])
            bits = pack.dynamic_bits(dy)[0]
            enc = T.DynamicBitsEncoder(rows, He).to(dev)
            static_enc = xavier(torch.nn.Conv1d(int(st.shape[1]), He, 1)).to(dev)
            if S["hm"]:
                C, W, L, m = S["hm"]
                dec_s, dec_d = xavier(torch.nn.Conv1d(D, Hd - m, 1)).to(dev), xavier(T.HeightmapEncoder(C, m, (W, L))).to(dev)
                dd = torch.randint(0, 51, (B, C, W, L), device=dev).float()
            else:
                flen = cs[0] - 1
                dec_s, dec_d = xavier(torch.nn.Conv1d(D, Hd // 2, 1)).to(dev), xavier(torch.nn.Conv1d(flen, Hd // 2, 1)).to(dev)
                dd = torch.randint(0, 51, (B, flen, 1), device=dev).float()
            ds = torch.randint(1, 6, (B, D, 1), device=dev).float()
            sh, hh = torch.randn(B, He, nR, device=dev), torch.tanh(torch.randn(1, B, Hd, device=dev))
            sd = T.StepDropout(11, dev)
            row = {"shape": S["name"], "B": B, "He": He, "Hd": Hd, "rows": rows, "nR": nR, "Ks": D, "map_m": S["hm"]}
            modules = (net, enc, dec_s, dec_d)

            def hidden_of(ds_, dd_, dec_s=dec_s, dec_d=dec_d, hm=S["hm"], B=B):
                return torch.cat((dec_s(ds_.reshape(B, -1, 1)), dec_d(dd_) if hm else dec_d(dd_.reshape(B, -1, 1))), 1)

            # (a) the launches alone
            with torch.no_grad():
                proj = net.project_static(sh)
                fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
                h_out, q_out = torch.empty(B, Hd, device=dev), torch.empty(B, Hd, device=dev)
                keep = torch.empty(B, 2, Hd // 64, dtype=torch.int64, device=dev)
                rec = sd.take_step(P_DROP, P_DROP)
                xs2, h2 = ds.view(B, D), hh[0]
                if S["hm"]:
                    ew = tuple(t.detach().reshape(t.shape[0], -1) if t.dim() == 4 else t.detach()
                               for cv in (dec_d.conv1, dec_d.conv2, dec_d.conv3) for t in (cv.weight, cv.bias))
                    tail = (fold.P, fold.c, fold.w_hh, fold.b_hh, fold.Wq)
                    plain = lambda: rollout._decoder_hm_into(xs2, dd, h2, ew, *tail, h_out, q_out, None, None)                       # noqa: E731
                    drop = lambda: rollout._decoder_hm_dropout_into(xs2, dd, h2, ew, *tail, rec, h_out, q_out, None, None, None, keep)  # noqa: E731
                else:
                    args_ = (xs2, dd.view(B, -1), h2, fold.P, fold.c, fold.w_hh, fold.b_hh, fold.Wq)
                    plain = lambda: rollout._decoder_into(*args_, h_out, q_out, None)                                                # noqa: E731
                    drop = lambda: rollout._decoder_dropout_into(*args_, rec, h_out, q_out, None, None, keep)                        # noqa: E731
                graphs = {"plain_launch": captured(plain, dev, per)[0], "dropout_launch": captured(drop, dev, per)[0]}
                res = alternate(graphs, args.runs, lambda g: replay_us(g, args.reps, per))
                row["a_launch_us"] = res
                row["a_generator_cost_us"] = round(statistics.median(res["dropout_launch"]) - statistics.median(res["plain_launch"]), 2)

                # (b) forward of one step
                f_ours = lambda: net.forward_step_dropout(proj, bits, fold, ds, dd, hh, sd)                                          # noqa: E731
                f_parent = lambda: net.forward_bits(proj, bits, enc, hidden_of(ds, dd), hh)                                          # noqa: E731
                res = alternate({"forward_step_dropout": f_ours, "convs_forward_bits": f_parent}, args.runs, lambda f: eager_us(f, args.reps))
                row["b_forward_us"] = res
                row["b_forward"] = summary(res, "forward_step_dropout", "convs_forward_bits")

            # (b) forward + backward of one step, to every leaf of each side
            g1, g2 = torch.randn(B, nR, device=dev), torch.randn(1, B, Hd, device=dev)
            leaf = lambda t: t.detach().clone().requires_grad_(True)                                                                 # noqa: E731
            fl = rollout_fold_leaves(fold, leaf)
            projl, h_ours, h_par, proj_par = leaf(proj), leaf(hh), leaf(hh), leaf(proj)
            proj_par.static_hidden = sh
            ours_leaves = [projl, h_ours] + [getattr(fl, k) for k in ("M", "k", "P", "c", "Wq", "va", "vp", "w_hh", "b_hh")] + \
                ([p for p in dec_d.parameters()] if S["hm"] else [])
            par_leaves = [proj_par, h_par] + [p for mod in modules for p in mod.parameters()]

            def fb_ours():
                logits, last = net.forward_step_dropout(projl, bits, fl, ds, dd, h_ours, sd)
                return torch.autograd.grad((logits * g1).sum() + (last * g2).sum(), ours_leaves, allow_unused=True)

            def fb_parent():
                logits, last = net.forward_bits(proj_par, bits, enc, hidden_of(ds, dd), h_par)
                return torch.autograd.grad((logits * g1).sum() + (last * g2).sum(), par_leaves, allow_unused=True)
            res = alternate({"forward_step_dropout": fb_ours, "convs_forward_bits": fb_parent}, args.runs, lambda f: eager_us(f, args.reps))
            row["b_forward_backward_us"] = res
            row["b_forward_backward"] = summary(res, "forward_step_dropout", "convs_forward_bits")
            rows_out.append(row)
            write()
            print(json.dumps(row), flush=True)

            # (c) the ten-step training episode with the head, forward + backward to every parameter
            u = torch.rand(n, B, device=dev)
            adv = torch.randn(B, device=dev)
            params = [p for mod in modules + (static_enc,) for p in mod.parameters()]
            sides = {}
            for label in ("forward_step_dropout", "convs_forward_bits"):
                env = T.BatchedContainer(B, cs, n, "C+P+S-lb-soft", "diff", device=dev)

                def ep(label=label, env=env):
                    with torch.enable_grad():
                        sp = T.EpisodeStepper(st, dy, env, expand_dynamic=False)
                        pr = net.project_static(static_enc(st))
                        state = {"hh": None}
                        if label == "forward_step_dropout":
                            sd.next_episode()
                            fo = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))

                            def scorer(step, decoder_static, decoder_dynamic, **_):
                                logits, state["hh"] = net.forward_step_dropout(pr, sp.dynamic_bits, fo, decoder_static, decoder_dynamic,
                                                                               state["hh"], sd)
                                return logits
                        else:
                            def scorer(step, decoder_static, decoder_dynamic, **_):
                                logits, state["hh"] = net.forward_bits(pr, sp.dynamic_bits, enc, hidden_of(decoder_static, decoder_dynamic),
                                                                       state["hh"])
                                return logits
                        pol = T.PointerHeadPolicy(scorer, u=u)
                        T.run_episode(st, dy, pol, cs[0], cs[-1], stepper=sp, check=False)
                        loss = (adv * pol.tour_logp().sum(1)).sum()
                        return torch.autograd.grad(loss, params, allow_unused=True)
                sides[label] = ep
            res = alternate(sides, args.runs, lambda f: eager_us(f, max(5, args.reps // 2)))
            row["c_episode_us"] = res
            row["c_episode"] = summary(res, "forward_step_dropout", "convs_forward_bits")
            write()
            print(json.dumps({"shape": S["name"], "c_episode": row["c_episode"]}), flush=True)
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    write()
    print("wrote", args.out)


def rollout_fold_leaves(fold, leaf):
    """a copy of a StepFold whose tensors are leaves (the per-episode folds' own backward is not a step's cost)"""
    from tap_net_amd.tools import StepFold
    out = StepFold()
    for k in StepFold.__slots__:
        v = getattr(fold, k)
        setattr(out, k, leaf(v) if torch.is_tensor(v) and v.is_floating_point() else v)
    return out


if __name__ == "__main__":
    main()
