#!/usr/bin/env python3
"""Time tools.DRL -- the module that owns the actor episode -- against the hand-wired recipe it replaces (INTEGRATION 2i /
2m; the episode scripts/time_decoder_dropout.py times in its section (c)): a BatchedContainer and a lean EpisodeStepper kept
across episodes, fold_static + fold_decoder + fold_episode, a scorer closure that threads last_hh, a PointerHeadPolicy,
run_episode, the stacked log-probabilities.  Both sides run on the SAME children in the same process, alternating.

Shapes: the c2 episode (B = 8 192, n = 10, He = Hd = 128) and the 3D actor of profiles/heightmap_step.json (B = 4 096, He 128,
Hd 256, the 2 x 5 x 5 map through a HeightmapEncoder of m = 128).

  (a) eval     the ten-step episode forward only, no_grad, greedy: DRL.forward against the recipe with
               PointerHeadPolicy(greedy=True)
  (b) train    the same episode in train() at p = 0.1, forward + backward to every parameter: DRL.forward (the head's DRAW
               launch) against the recipe with a StepDropout for the masks and PRE-DRAWN uniforms for the head, as
               time_decoder_dropout.py runs it
  (c) head     the DRAW launch against torch.rand + the sampling launch, ``--per-call`` of them back to back per timed call

All three run eagerly, as a training loop does -- device events around the call, one synchronisation per repetition (torch's
own generator is not captured in a graph here: the package's notes record aborts under back-to-back replays).  Every
figure is the median of ``--reps`` repetitions after warm-ups; each side is measured ``--runs`` times after one discarded round, the sides alternating
in an order that reverses every round, and the row keeps every run: the spread is max - min of a side's runs.  Writes profiles/drl.json, rewritten after every row.

    python scripts/time_drl.py [--reps 20] [--runs 4] [--per-call 8] [--only SHAPE] [--out profiles/drl.json]
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

P_DROP = 0.1
SHAPES = [dict(name="c2_Hd128", D=2, B=8192, He=128, Hd=128, cs=[5, 50]),
          dict(name="c3_heightmap_Hd256", D=3, B=4096, He=128, Hd=256, cs=[5, 5, 50])]


def alternate(sides, runs, clock):
    """{label: fn} -> {label: [median of each run]}: one discarded round first (the first timed call of a process also pays
    for allocator growth and clock ramp), then ``runs`` rounds, the order of the sides reversed on every other round"""
    for s in sides.values():
        clock(s)
    out = {k: [] for k in sides}
    for r in range(runs):
        for k in (list(sides) if r % 2 == 0 else list(sides)[::-1]):
            out[k].append(round(clock(sides[k]), 2))
    return out


def summary(res, ours, recipe):
    """median and spread (max - min) of both sides' runs; the module's excess over the recipe and whether it lies within the
    recipe's own run-to-run spread"""
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: round(max(v) - min(v), 2) for k, v in res.items()}
    excess = med[ours] - med[recipe]
    return {"median_us": med, "spread_us": spread, "module_minus_recipe_us": round(excess, 2),
            "ratio": round(med[ours] / med[recipe], 4), "within_recipe_spread": bool(excess <= spread[recipe])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--per-call", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drl.json"))
    ap.add_argument("--only", default=None, help="measure this shape alone")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    per, rows_out, n = args.per_call, [], 10

    def write():
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "p": P_DROP,
                       "note": "device events around eager calls, one synchronisation per repetition; (c): %d head calls per timed call, "
                               "divided out; medians of %d repetitions, %d runs per side, sides alternating; "
                               "spread = max - min of a side's runs; microseconds" % (per, args.reps, args.runs),
                       "rows": rows_out}, f, indent=1)
    pack.set_binary_check('trust')
    torch.manual_seed(3)
    try:
        for S in (S for S in SHAPES if args.only in (None, S["name"])):
            D, B, He, Hd, cs = S["D"], S["B"], S["He"], S["Hd"], S["cs"]
            actor = T.DRL(D, 3 * n, He, Hd, True, 'bot', True, cs[0], cs[-1], D, "C+P+S-lb-soft", 'shape_heightmap', 'diff', 'LB_GREEDY',
                          pack.update_dynamic, pack.update_mask, 1, P_DROP, seed=11).to(dev)
            st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
            nR = int(dy.shape[2])
            zeros = (torch.zeros(B, D, 1, device=dev), torch.zeros((B, cs[0] - 1, 1) if D == 2 else (B, 2, cs[0], cs[1]), device=dev))
            adv = torch.randn(B, device=dev)
            u = torch.rand(n, B, device=dev)
            params = list(actor.parameters())
            pointer = actor.pointer
            env = T.BatchedContainer(B, cs, n, "C+P+S-lb-soft", "diff", device=dev)
            sp = T.EpisodeStepper(st, dy, env, steps=n, expand_dynamic=False)
            sd = T.StepDropout(11, dev)
            row = {"shape": S["name"], "B": B, "n": n, "He": He, "Hd": Hd, "rows": int(dy.shape[1]), "nR": nR}

            def recipe(train):
                state = {"hh": None}
                if train:
                    sd.next_episode()
                sf = pointer.fold_static(actor.static_encoder, st[:, 1:, :])
                fold = pointer.fold_episode(actor.dynamic_encoder, *pointer.fold_decoder(actor.static_decoder, actor.dynamic_decoder))

                def scorer(step, decoder_static, decoder_dynamic, **_):
                    if train:
                        logits, state["hh"] = pointer.forward_step_dropout(sf, sp.dynamic_bits, fold, decoder_static, decoder_dynamic,
                                                                           state["hh"], sd)
                    else:
                        logits, state["hh"] = pointer.forward_step(sf, sp.dynamic_bits, fold, decoder_static, decoder_dynamic, state["hh"])
                    return logits
                pol = T.PointerHeadPolicy(scorer, u=u) if train else T.PointerHeadPolicy(scorer, greedy=True)
                out = T.run_episode(st, dy, pol, cs[0], cs[-1], stepper=sp)
                return out["tour_idx"], pol.tour_logp(), out["reward"]

            # (a) eval, forward only
            actor.eval()

            def module_eval():
                with torch.no_grad():
                    return actor(st, dy, zeros)

            def recipe_eval():
                with torch.no_grad():
                    return recipe(False)
            a, b = module_eval(), recipe_eval()
            row["a_same_bytes"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[2]))
            res = alternate({"module": module_eval, "recipe": recipe_eval}, args.runs, lambda f: eager_us(f, args.reps))
            row["a_eval_forward_us"] = res
            row["a_eval_forward"] = summary(res, "module", "recipe")
            rows_out.append(row)
            write()

            # (b) train at p = 0.1, forward + backward to every parameter
            actor.train()

            def module_train():
                with torch.enable_grad():
                    out = actor(st, dy, zeros)
                    return torch.autograd.grad((adv * out[1].sum(1)).sum(), params, allow_unused=True)

            def recipe_train():
                with torch.enable_grad():
                    out = recipe(True)
                    return torch.autograd.grad((adv * out[1].sum(1)).sum(), params, allow_unused=True)
            res = alternate({"module": module_train, "recipe": recipe_train}, args.runs, lambda f: eager_us(f, max(5, args.reps // 2)))
            row["b_train_forward_backward_us"] = res
            row["b_train_forward_backward"] = summary(res, "module", "recipe")
            write()

            # (c) the head alone: DRAW against torch.rand + the sampling launch
            with torch.no_grad():
                logits, mask = torch.randn(B, nR, device=dev) * 3, (torch.rand(B, nR, device=dev) < 0.3).float()
                mask[:, 0] = 1
                rec = sd.take_pick()
                uu = torch.empty(B, device=dev)
                def draw():
                    for _ in range(per):
                        T.pointer_pick_draw(logits, mask, rec)

                def rand_then_sample():
                    for _ in range(per):
                        torch.rand(B, out=uu)
                        T.pointer_pick(logits, mask, uu)

                def sample_alone():
                    for _ in range(per):
                        T.pointer_pick(logits, mask, uu)
                res = alternate({"draw": draw, "rand_then_sample": rand_then_sample, "sample_alone": sample_alone}, args.runs,
                                lambda f: round(eager_us(f, args.reps) / per, 3))
            row["c_head_us"] = res
            row["c_head"] = {"median_us": {k: statistics.median(v) for k, v in res.items()},
                             "spread_us": {k: round(max(v) - min(v), 2) for k, v in res.items()}}
            write()
            print(json.dumps(row), flush=True)
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    write()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
