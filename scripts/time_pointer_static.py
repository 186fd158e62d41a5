#!/usr/bin/env python3
"""Time the pointer network's static-rows form (pointer.hip: tap_pointer_scores_static -- the static term of U computed from
the S rows of ``static`` inside the launch) against the ``proj`` form of the same library (tap_pointer_scores).  B = 8 192;
c2 (30, 20) with S = 2 at Hd = 128, c3 (30, 60) with S = 3 at Hd = 128 and at Hd = 256; He = Hd; the instances' own shadow.
Per shape, each row ``proj`` form against static-rows form:

  forward            the forward launch alone on kept buffers
  backward           the backward launch (+ its reduce) alone
  fwd_bwd            forward + backward()  from the step's leaves through autograd -- on the ``proj`` side ``proj`` is a leaf that
                     requires grad, so the accumulation of dproj into proj.grad is inside; on the static side dG's batched product
  prologue           the per-episode prologue, forward and backward: static_encoder + project_static (cotangent: a proj-sized
                     tensor) against fold_static (cotangents: dG, dg)

and on c2 the ten-step training episode with the head (pointer_pick from pre-drawn u) on a lean stepper, forward + backward to
every parameter, with torch.cuda.max_memory_allocated (reset before each side), and on the greedy episode the number of picks
that differ between the two forms (P by an fmaf chain and proj by a GEMM round differently: a near-tie may differ).

Clock: device events around a replay of a hipGraph holding ``--per-graph`` calls, after warm-ups; every figure is the median
of ``--reps`` replays, the sides alternating, two runs each (time_dyn_encoder.captured / two_runs).  The training episode
builds its stepper inside and runs eagerly, as a training loop does: device events around the call, one synchronisation per
repetition.  No speed bar: the numbers are recorded as they come out.  Writes profiles/pointer_static.json, rewritten after
every row.  Usage:

    python scripts/time_pointer_static.py [--reps 30] [--per-graph 4] [--out profiles/pointer_static.json]
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
from tap_net_amd import _lib, pack, rollout, synth  # noqa: E402
from time_dyn_encoder import captured, two_runs  # noqa: E402

B = 8192
SHAPES = [("c2_Hd128", 2, 10, [5, 50], 128), ("c3_Hd128", 3, 10, [5, 5, 50], 128), ("c3_Hd256", 3, 10, [5, 5, 50], 256)]


def xavier(m):
    for p in m.parameters():
        torch.nn.init.xavier_uniform_(p) if p.dim() > 1 else torch.nn.init.normal_(p, std=0.1)
    return m


def eager_us(fn, reps):
    for _ in range(2):
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
    return round(statistics.median(ts), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--per-graph", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointer_static.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    per, rows_out = args.per_graph, []

    def write(episode=None):
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev),
                       "note": "both sides are this library; launch / fwd_bwd / prologue rows: device events around hipGraph replays "
                               "(%d calls per graph), medians of %d replays after warm-ups, two runs each, sides alternating; the "
                               "training episode: eager, device events around the call, medians; microseconds" % (per, args.reps),
                       "rows": rows_out, "episode": episode}, f, indent=1)

    pack.set_binary_check('trust')
    P = _lib.ptr
    try:
        for name, D, n, cs, H in SHAPES:
            torch.manual_seed(3)
            net = xavier(T.Pointer(H, H, 'shape_heightmap', 'bot', dropout=0.0)).to(dev).eval()
            st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
            rows, nR, S = int(dy.shape[1]), int(dy.shape[2]), D
            bits = pack.dynamic_bits(dy)[0]
            enc = T.DynamicBitsEncoder(rows, H).to(dev)
            senc = torch.nn.Conv1d(S, H, 1).to(dev)
            xs = st[:, 1:, :].contiguous()
            row = {"shape": name, "B": B, "He": H, "Hd": H, "rows": rows, "nR": nR, "S": S, "proj_bytes": B * 3 * H * nR * 4,
                   "static_hidden_bytes": B * H * nR * 4, "xs_bytes": B * S * nR * 4, "dU_bytes": B * 3 * H * nR * 4,
                   "shadow_bytes": bits.numel() * 8}
            with torch.no_grad():
                proj = net.project_static(senc(xs))
                sf = net.fold_static(senc, xs)
                G, g = sf.G.contiguous(), sf.g.contiguous()
                _, Wd, Wq = (w.detach() for w in net.folded_weights())
                va, vp = net.encoder_attn.v[0, 0].detach(), net.v[0, 0].detach()
                Mf, k = Wd.matmul(enc.conv.weight[:, :, 0]).contiguous(), Wd.matmul(enc.conv.bias).contiguous()
                q = torch.tanh(torch.randn(B, H, device=dev)).matmul(Wq.t()).contiguous()
                o1 = [torch.empty(B, nR, device=dev), torch.empty(B, nR, device=dev), torch.empty(B, H, device=dev)]
                o2 = [torch.empty_like(t) for t in o1]
                f_proj = lambda: rollout._scores_into(proj, bits, Mf, k, q, va, vp, rows, *o1)                       # noqa: E731
                f_stat = lambda: rollout._scores_static_into(xs, bits, G, g, Mf, k, q, va, vp, rows, *o2)            # noqa: E731
                f_proj(), f_stat()
                row["max_abs_diff_logits"] = float((o1[0] - o2[0]).abs().max())
                row["forward_us"] = two_runs({"proj": captured(f_proj, dev, per)[0], "static": captured(f_stat, dev, per)[0]}, args.reps, per)
            rows_out.append(row)
            write()
            # the backward launches alone
            Lb, c = _lib.lib(), _lib.ctx(dev)
            need = max(int(Lb.tap_pointer_scores_backward_scratch(B, nR, rows, H)),
                       int(Lb.tap_pointer_scores_static_backward_scratch(B, nR, rows, H, S)))
            scratch = torch.empty(need // 4, device=dev)
            gr = torch.randn(B, nR, device=dev)
            dU, dq, dva, dvp = torch.empty(B, 3 * H, nR, device=dev), torch.empty(B, H, device=dev), torch.empty(H, device=dev), torch.empty(H, device=dev)

            def b_proj():
                _lib.check(Lb.tap_pointer_scores_backward(c, P(proj), P(bits), B, nR, rows, H, P(Mf), P(k), P(q), P(va), P(vp), P(o1[1]),
                                                          P(o1[2]), P(gr), P(dU), P(dq), P(dva), P(dvp), P(scratch), need, _lib.stream_of(dev)), c)

            def b_stat():
                _lib.check(Lb.tap_pointer_scores_static_backward(c, P(xs), P(bits), B, nR, rows, H, S, P(G), P(g), P(Mf), P(k), P(q), P(va),
                                                                 P(vp), P(o2[1]), P(o2[2]), P(gr), P(dU), P(dq), P(dva), P(dvp), P(scratch),
                                                                 need, _lib.stream_of(dev)), c)
            row["backward_us"] = two_runs({"proj": captured(b_proj, dev, per)[0], "static": captured(b_stat, dev, per)[0]}, args.reps, per)
            write()
            del dU
            # forward + backward() from the step's leaves: .grad accumulates, as it does over an episode's steps
            leaf = lambda t: t.detach().clone().requires_grad_(True)                                                 # noqa: E731
            L1 = [leaf(t) for t in (proj, Mf, k, q, va, vp)]
            L2 = [leaf(t) for t in (G, g, Mf, k, q, va, vp)]
            fb = {"proj": lambda: (T.pointer_scores(L1[0], bits, *L1[1:], rows=rows) * gr).sum().backward(),
                  "static": lambda: (T.pointer_scores_static(xs, bits, *L2, rows=rows) * gr).sum().backward()}
            graphs = {}
            for label, fn in fb.items():
                try:
                    graphs[label] = captured(fn, dev, per)[0]
                except RuntimeError as e:                                            # a side that does not capture is recorded as such
                    row["fwd_bwd_%s_error" % label] = str(e).splitlines()[0][:200]
                    torch.cuda.synchronize()
            row["fwd_bwd_us"] = two_runs(graphs, args.reps, per)
            write()
            del graphs, L1, L2
            # the per-episode prologue, forward and backward
            dproj, dG, dg = torch.randn_like(proj), torch.randn_like(G), torch.randn_like(g)
            pp = [net.W, net.encoder_attn.W, senc.weight, senc.bias]

            def p_proj():
                return torch.autograd.grad(net.project_static(senc(xs)), pp, dproj)

            def p_stat():
                f = net.fold_static(senc, st[:, 1:, :])
                return torch.autograd.grad((f.G, f.g), pp, (dG, dg))
            row["prologue_us"] = two_runs({"proj": captured(p_proj, dev, per)[0], "static": captured(p_stat, dev, per)[0]}, args.reps, per)
            print(json.dumps(row), flush=True)
            write()
            del proj, dproj
            torch.cuda.empty_cache()

        # the ten-step c2 training episode with the head, forward + backward to every parameter
        name, D, n, cs, H = SHAPES[0]
        torch.manual_seed(5)
        net = xavier(T.Pointer(H, H, 'shape_heightmap', 'bot', dropout=0.0)).to(dev).eval()
        st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
        rows, nR = int(dy.shape[1]), int(dy.shape[2])
        enc, senc = T.DynamicBitsEncoder(rows, H).to(dev), torch.nn.Conv1d(D, H, 1).to(dev)
        dec_s, dec_d = torch.nn.Conv1d(D, H // 2, 1).to(dev), torch.nn.Conv1d(4, H // 2, 1).to(dev)
        u, adv = torch.rand(n, B, device=dev), torch.randn(B, device=dev)
        params = [p for m in (net, enc, senc, dec_s, dec_d) for p in m.parameters()]

        def episode(label, greedy=False):
            env = T.BatchedContainer(B, cs, n, "C+P+S-lb-soft", "diff", device=dev)
            sp = T.EpisodeStepper(st, dy, env, expand_dynamic=False)
            pr = net.fold_static(senc, st[:, 1:, :]) if label == "static" else net.project_static(senc(st[:, 1:, :]))
            fo = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
            state = {"hh": None}

            def scorer(step, decoder_static, decoder_dynamic, **_):
                logits, state["hh"] = net.forward_step(pr, sp.dynamic_bits, fo, decoder_static, decoder_dynamic, state["hh"])
                return logits
            pol = T.PointerHeadPolicy(scorer, greedy=True) if greedy else T.PointerHeadPolicy(scorer, u=u)
            out = T.run_episode(st, dy, pol, cs[0], cs[-1], stepper=sp, check=False)
            if greedy:
                return out["tour_idx"].clone()
            return torch.autograd.grad((adv * pol.tour_logp().sum(1)).sum(), params, allow_unused=True)
        ep = {"window": "c2", "B": B, "He": H, "Hd": H, "steps": n, "training_episode_us": {"proj": [], "static": []}, "peak_bytes": {}}
        for label in ("proj", "static"):
            with torch.enable_grad():
                episode(label)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            with torch.enable_grad():
                episode(label)
            torch.cuda.synchronize()
            ep["peak_bytes"][label] = {"before": base, "peak": torch.cuda.max_memory_allocated(dev)}
        for _ in range(2):
            for label in ("proj", "static"):
                with torch.enable_grad():
                    ep["training_episode_us"][label].append(eager_us(lambda: episode(label), max(5, args.reps // 3)))
        with torch.no_grad():
            tours = {label: episode(label, greedy=True) for label in ("proj", "static")}
        ep["greedy_picks"] = int(tours["proj"].numel())
        ep["greedy_picks_that_differ"] = int((tours["proj"] != tours["static"]).sum().item())
        print(json.dumps(ep), flush=True)
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    write(ep)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
