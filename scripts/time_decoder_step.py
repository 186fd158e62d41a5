#!/usr/bin/env python3
"""Time the decoder step (decoder.hip: tap_decoder_step, one launch) against the torch form of the same lines of the
loop (model.py:347-354 and the GRU step and q of tools.Pointer.forward_bits), piece by piece.  B = 8 192, He = Hd = 128,
windows c2 (rows 30, nR 20; decoder values 2 + 4) and c3 (rows 30, nR 60; 3 + 50), two Conv1d decoder encoders of Hd / 2
rows each, concatenated.  Forward, per decoding step:

  decoder_step_kernel   the launch alone on kept buffers, h given
  convs_cat             the two decoder convolutions and their concatenation
  nn_gru                tools.Pointer._gru_step: the transpose, nn.GRU for one step, the two dropouts (p = 0)
  q                     rnn_out . Wq^T
  M_k                   forward_bits' per-step products for M and k (folded_weights' concatenations included)
  forward_step          tools.Pointer.forward_step: decoder_step + pointer_scores
  convs_forward_bits    the parent's path: convs_cat, then tools.Pointer.forward_bits

Forward + backward from the step's leaves: ``decoder_step`` under autograd (leaves P, c, w_hh, b_hh, wq, h) against
convolutions + nn.GRU + q under torch autograd (leaves: the encoders' and the GRU's parameters, Wq, h).

Then the ten-step c2 episode from a hipGraph with pointer_pick (greedy) on lean steppers: a forward_step scorer against
convolutions + forward_bits; the two tours are compared.

Clock: device events around a replay of a hipGraph holding ``--per-graph`` calls (one episode for the episode rows), after
warm-ups; every figure is the median of ``--reps`` replays, the sides alternating, two runs each.  Writes
profiles/decoder_step.json, rewritten after every row.  Usage:

    python scripts/time_decoder_step.py [--reps 30] [--per-graph 4] [--out profiles/decoder_step.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tap_net_amd as T  # noqa: E402
from tap_net_amd import pack, rollout, synth  # noqa: E402
from time_dyn_encoder import captured, two_runs  # noqa: E402

B, H = 8192, 128
WINDOWS = [("c2", 2, 10, [5, 50]), ("c3", 3, 10, [5, 5, 50])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--per-graph", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    per = args.per_graph
    rows_out, later, episode = [], [], None

    def write(episode=None):
        """the file as it stands: rewritten after every row, so a run that is cut short leaves the rows it measured"""
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev),
                       "note": "device events around hipGraph replays (%d calls per graph, one episode for the episode rows), "
                               "medians of %d replays after warm-ups, two runs each, sides alternating; microseconds" % (per, args.reps),
                       "rows": rows_out, "episode": episode}, f, indent=1)

    def xavier(m):
        for p in m.parameters():
            torch.nn.init.xavier_uniform_(p) if p.dim() > 1 else torch.nn.init.normal_(p, std=0.1)
        return m
    torch.manual_seed(3)
    net = xavier(T.Pointer(H, H, 'shape_heightmap', 'bot', dropout=0.0)).to(dev).eval()
    pack.set_binary_check('trust')
    try:
        for name, D, n, cs in WINDOWS:
            st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
            rows, nR = int(dy.shape[1]), int(dy.shape[2])
            bits = pack.dynamic_bits(dy)[0]
            flen = cs[0] - 1 if D == 2 else 2 * cs[0] * cs[1]
            enc = T.DynamicBitsEncoder(rows, H).to(dev)
            dec_s, dec_d = xavier(torch.nn.Conv1d(D, H // 2, 1)).to(dev), xavier(torch.nn.Conv1d(flen, H // 2, 1)).to(dev)
            sh, hh = torch.randn(B, H, nR, device=dev), torch.tanh(torch.randn(1, B, H, device=dev))
            ds = torch.randint(1, 6, (B, D, 1), device=dev).float()
            dd = torch.randint(0, 51, (B, flen, 1), device=dev).float()
            row = {"window": name, "B": B, "He": H, "Hd": H, "rows": rows, "nR": nR, "Ks": D, "Kd": flen,
                   "kernel_bytes_per_step": 4 * (B * (D + flen + 3 * H) + 4 * H * H + 3 * H * (D + flen + 2))}
            with torch.no_grad():
                proj = net.project_static(sh)
                fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
                Wq = fold.Wq

                def f_convs():
                    return torch.cat((dec_s(ds), dec_d(dd)), 1)
                hidden = f_convs()
                rnn_out = net._gru_step(hidden, hh)[0]
                h_out, q_out = torch.empty(B, H, device=dev), torch.empty(B, H, device=dev)
                xs2, xd2, h2 = ds.view(B, D), dd.view(B, flen), hh[0]

                def f_kernel():
                    rollout._decoder_into(xs2, xd2, h2, fold.P, fold.c, fold.w_hh, fold.b_hh, Wq, h_out, q_out, None)

                def f_gru():
                    return net._gru_step(hidden, hh)

                def f_q():
                    return rnn_out.matmul(Wq.t())

                def f_mk():
                    _, Wd, _ = net.folded_weights()
                    return Wd.matmul(enc.conv.weight[:, :, 0]), Wd.matmul(enc.conv.bias)

                def f_step():
                    return net.forward_step(proj, bits, fold, ds, dd, hh)

                def f_parent():
                    return net.forward_bits(proj, bits, enc, f_convs(), hh)
                a, b = f_step(), f_parent()
                row["max_abs_diff_vs_parent"] = {"logits": float((a[0] - b[0]).abs().max()), "last_hh": float((a[1] - b[1]).abs().max())}
                graphs = {k: captured(f, dev, per)[0] for k, f in (
                    ("decoder_step_kernel", f_kernel), ("convs_cat", f_convs), ("nn_gru", f_gru), ("q", f_q), ("M_k", f_mk),
                    ("forward_step", f_step), ("convs_forward_bits", f_parent))}
                row.update({k + "_us": v for k, v in two_runs(graphs, args.reps, per).items()})
            rows_out.append(row)
            write()
            print(json.dumps(row), flush=True)

            def fwd_bwd(row=row, fold=fold, Wq=Wq, hh=hh, ds=ds, dd=dd, dec_s=dec_s, dec_d=dec_d):
                """forward + backward from the step's leaves (run last: the GRU's backward under capture is the one
                piece here that no other script of the project has captured)"""
                g1, g2 = torch.randn(B, H, device=dev), torch.randn(B, H, device=dev)
                leaf = lambda t: t.detach().clone().requires_grad_(True)                              # noqa: E731
                L1 = [leaf(t) for t in (hh[0], fold.P, fold.c, fold.w_hh, fold.b_hh, Wq)]
                net.train()                                                  # (the GRU's device backward exists in training mode only; p = 0)
                wq2, h0 = leaf(Wq), leaf(hh)
                params = list(dec_s.parameters()) + list(dec_d.parameters()) + list(net.gru.parameters())

                def fb_kernel():
                    hn, q = T.decoder_step(ds, dd, *L1)
                    return torch.autograd.grad((hn * g1).sum() + (q * g2).sum(), L1)

                def fb_parent():
                    rnn, last = net._gru_step(torch.cat((dec_s(ds), dec_d(dd)), 1), h0)
                    return torch.autograd.grad((last[0] * g1).sum() + (rnn.matmul(wq2.t()) * g2).sum(), params + [wq2, h0])
                graphs = {}
                for label, fn in (("decoder_step", fb_kernel), ("convs_gru_q", fb_parent)):
                    try:
                        graphs[label] = captured(fn, dev, per)[0]
                    except RuntimeError as e:                                 # a side that does not capture is recorded as such
                        row["fwd_bwd_" + label + "_error"] = str(e).splitlines()[0][:200]
                        torch.cuda.synchronize()
                row.update({"fwd_bwd_" + k + "_us": v for k, v in two_runs(graphs, args.reps, per).items()})
                net.eval()
                print(json.dumps(row), flush=True)
                write(episode)
            later.append(fwd_bwd)
        # the ten-step c2 episode from a hipGraph with the head, both sides on lean steppers
        name, D, n, cs = WINDOWS[0]
        st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
        rows, nR = int(dy.shape[1]), int(dy.shape[2])
        enc = T.DynamicBitsEncoder(rows, H).to(dev)
        dec_s, dec_d = xavier(torch.nn.Conv1d(D, H // 2, 1)).to(dev), xavier(torch.nn.Conv1d(cs[0] - 1, H // 2, 1)).to(dev)
        sh, hh0 = torch.randn(B, H, nR, device=dev), torch.zeros(1, B, H, device=dev)
        graphs, keeps = {}, {}
        with torch.no_grad():
            proj = net.project_static(sh)
            fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
            for label in ("forward_step", "convs_forward_bits"):
                env = T.BatchedContainer(B, cs, n, "C+P+S-lb-soft", "diff", device=dev)
                sp = T.EpisodeStepper(st, dy, env, 'bot', True, steps=n, expand_dynamic=False)
                state = {}

                def scorer(step, decoder_static, decoder_dynamic, sp=sp, state=state, label=label, **_):
                    if label == "forward_step":
                        logits, state["hh"] = net.forward_step(proj, sp.dynamic_bits, fold, decoder_static, decoder_dynamic,
                                                               None if step == 0 else state["hh"])
                    else:
                        hidden = torch.cat((dec_s(decoder_static), dec_d(decoder_dynamic)), 1)
                        logits, state["hh"] = net.forward_bits(proj, sp.dynamic_bits, enc, hidden, hh0 if step == 0 else state["hh"])
                    return logits
                pol = T.PointerHeadPolicy(scorer, greedy=True)

                def ep(sp=sp, pol=pol):
                    out = T.run_episode(st, dy, pol, cs[0], cs[-1], stepper=sp, check=False)
                    return out["tour_idx"], out["reward"], pol.tour_logp()
                graphs[label], keeps[label] = captured(ep, dev)
            res = two_runs(graphs, args.reps, 1)
        same = float((keeps["forward_step"][0] == keeps["convs_forward_bits"][0]).float().mean().item())
        episode = {"window": "c2", "B": B, "He": H, "Hd": H, "steps": n, "picks_equal": round(same, 5),
                   "tours_identical": bool(torch.equal(keeps["forward_step"][0], keeps["convs_forward_bits"][0])),
                   "max_abs_diff_tour_logp": float((keeps["forward_step"][2] - keeps["convs_forward_bits"][2]).abs().max())}
        episode.update({k + "_episode_us": t for k, t in res.items()})
        print(json.dumps(episode), flush=True)
        write(episode)
        for fn in later:
            fn()
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    write(episode)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
