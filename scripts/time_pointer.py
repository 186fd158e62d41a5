#!/usr/bin/env python3
"""Time the pointer network on the bit shadow (pointer.hip: tap_pointer_scores, one launch) against the two torch forms
of the same line of the loop (model.py:356-358).  B = 8 192, He = Hd = 128, windows (rows, nR) = (30, 20) [c2] and
(30, 60) [c3]; the instances' own shadow (about 9 % ones).  Forward, each side one decoding step with its GRU step:

  forward_bits       tools.Pointer.forward_bits: GRU, the fold of the encoder into the two W (M, k), q, the launch
  reference          DynamicBitsEncoder(bits) + tools.Pointer.forward: the reference's concatenations and bmm
  folded_torch       GRU, M, k, q, then U = proj + k + M . dynamic (on the fp32 `dynamic`) and the rest in plain torch
  scores_kernel      the launch alone on kept buffers (what the byte counts of DESIGN 7f are set against)

Forward + backward, from the step's leaf tensors (no GRU: its backward is the same on every side): ``pointer_scores``
under autograd (the backward launches), the reference form and the folded torch form under torch autograd; and the
backward launches alone (tap_pointer_scores_backward + tap_encode_bits_backward on dU).

Then the ten-step c2 episode from a hipGraph with pointer_pick, on lean steppers: a forward_bits scorer against
DynamicBitsEncoder + forward.

Clock: device events around a replay of a hipGraph holding ``--per-graph`` calls (one episode for the episode rows),
after warm-ups; every figure is the median of ``--reps`` replays, the sides alternating, two runs each.  No speed bar:
the numbers are recorded as they come out.  Writes profiles/pointer.json, rewritten after every row.  Usage:

    python scripts/time_pointer.py [--reps 30] [--per-graph 4] [--out profiles/pointer.json]
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
from tap_net_amd import _lib, pack, rollout, synth  # noqa: E402
from time_dyn_encoder import captured, two_runs  # noqa: E402

B, H = 8192, 128
WINDOWS = [("c2", 2, 10, [5, 50]), ("c3", 3, 10, [5, 5, 50])]


def folded_torch(proj3, dyn, M, k, q, va, vp):
    """the contract in plain torch on proj (B, 3 Hd, nR) and the fp32 0/1 ``dyn``"""
    Hd = q.shape[1]
    U = proj3 + k[None, :, None] + torch.einsum('xr,brc->bxc', M, dyn)
    attn = torch.softmax(torch.einsum('j,bjc->bc', va, torch.tanh(U[:, :Hd] + q[:, :, None])), dim=1)
    t = torch.einsum('bc,bjc->bj', attn, U[:, 2 * Hd:])
    return torch.einsum('j,bjc->bc', vp, torch.tanh(U[:, Hd:2 * Hd] + t[:, :, None]))


def reference_scores(net, sh, dh, rnn_out):
    """tools.Pointer.forward after its GRU step"""
    Bn, nR = sh.size(0), sh.shape[-1]
    enc = torch.cat((sh, dh), 1)
    hidden = torch.cat((enc, rnn_out.unsqueeze(2).repeat(1, 1, nR)), 1)
    at = net.encoder_attn
    attn = torch.softmax(torch.bmm(at.v.expand(Bn, 1, -1), torch.tanh(torch.bmm(at.W.expand(Bn, -1, -1), hidden))), dim=2)
    context = attn.bmm(enc.permute(0, 2, 1)).transpose(1, 2).expand_as(enc)
    energy = torch.cat((enc, context), dim=1)
    return torch.bmm(net.v.expand(Bn, -1, -1), torch.tanh(torch.bmm(net.W.expand(Bn, -1, -1), energy))).squeeze(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--per-graph", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointer.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    per = args.per_graph
    rows_out = []

    def write(episode=None):
        """the file as it stands: rewritten after every row, so a run that is cut short leaves the rows it measured"""
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev),
                       "note": "device events around hipGraph replays (%d calls per graph, one episode for the episode rows), "
                               "medians of %d replays after warm-ups, two runs each, sides alternating; microseconds" % (per, args.reps),
                       "rows": rows_out, "episode": episode}, f, indent=1)

    torch.manual_seed(3)
    net = T.Pointer(H, H, 'shape_heightmap', 'bot', dropout=0.0).to(dev)
    for p in net.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_uniform_(p)
    pack.set_binary_check('trust')
    try:
        for name, D, n, cs in WINDOWS:
            st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
            rows, nR = int(dy.shape[1]), int(dy.shape[2])
            bits = pack.dynamic_bits(dy)[0]
            enc = T.DynamicBitsEncoder(rows, H).to(dev)
            sh, dec, hh = torch.randn(B, H, nR, device=dev), torch.randn(B, H, 1, device=dev), torch.randn(1, B, H, device=dev)
            row = {"window": name, "B": B, "He": H, "Hd": H, "rows": rows, "nR": nR, "proj_bytes": B * 3 * H * nR * 4,
                   "shadow_bytes": bits.numel() * 8, "ones_share": round(float(dy.mean().item()), 4),
                   "reference_concat_bytes": B * nR * 4 * (3 * H + 4 * H)}
            net.eval()
            with torch.no_grad():
                proj = net.project_static(sh)
                proj3 = proj.permute(0, 1, 3, 2).reshape(B, 3 * H, nR).contiguous()
                Ws, Wd, Wq = (w.detach() for w in net.folded_weights())
                va, vp = net.encoder_attn.v[0, 0].detach(), net.v[0, 0].detach()

                def f_bits():
                    return net.forward_bits(proj, bits, enc, dec, hh)

                def f_ref():
                    return net(sh, enc(bits), dec, hh)

                def f_fold():
                    rnn_out, last = net._gru_step(dec, hh)
                    Mf, k = Wd.matmul(enc.conv.weight[:, :, 0]), Wd.matmul(enc.conv.bias)
                    return folded_torch(proj3, dy, Mf, k, rnn_out.matmul(Wq.t()), va, vp), last
                a, b, c = f_bits()[0], f_ref()[0], f_fold()[0]
                row["max_abs_diff_vs_reference"] = {"forward_bits": float((a - b).abs().max()), "folded_torch": float((c - b).abs().max())}
                Mf, k = Wd.matmul(enc.conv.weight[:, :, 0]).contiguous(), Wd.matmul(enc.conv.bias).contiguous()
                q = net._gru_step(dec, hh)[0].matmul(Wq.t()).contiguous()
                outs = [torch.empty(B, nR, device=dev), torch.empty(B, nR, device=dev), torch.empty(B, H, device=dev)]
                f_kernel = lambda: rollout._scores_into(proj, bits, Mf, k, q, va, vp, rows, *outs)    # noqa: E731
                graphs = {"forward_bits": captured(f_bits, dev, per)[0], "reference": captured(f_ref, dev, per)[0],
                          "folded_torch": captured(f_fold, dev, per)[0], "scores_kernel": captured(f_kernel, dev, per)[0]}
                row.update({k2 + "_us": v for k2, v in two_runs(graphs, args.reps, per).items()})
            rows_out.append(row)
            write()
            # forward + backward from the step's leaves
            g = torch.randn(B, nR, device=dev)
            leaf = lambda t: t.detach().clone().requires_grad_(True)                              # noqa: E731
            L1 = [leaf(t) for t in (proj, Mf, k, q, va, vp)]
            L2 = [leaf(t) for t in (proj3, Mf, k, q, va, vp)]
            dh = enc(bits).detach()
            L3 = [leaf(sh), leaf(dh), leaf(q)]
            params = [net.W, net.v, net.encoder_attn.W, net.encoder_attn.v]
            fb = {"pointer_scores": lambda: torch.autograd.grad((T.pointer_scores(L1[0], bits, *L1[1:], rows=rows) * g).sum(), L1),
                  "folded_torch": lambda: torch.autograd.grad((folded_torch(L2[0], dy, *L2[1:]) * g).sum(), L2),
                  "reference": lambda: torch.autograd.grad((reference_scores(net, *L3) * g).sum(), L3 + params)}
            graphs = {}
            for label, fn in fb.items():
                try:
                    graphs[label] = captured(fn, dev, per)[0]
                except RuntimeError as e:                                                          # a side that does not capture is recorded as such
                    row["fwd_bwd_" + label + "_error"] = str(e).splitlines()[0][:200]
                    torch.cuda.synchronize()
            row.update({"fwd_bwd_" + k2 + "_us": v for k2, v in two_runs(graphs, args.reps, per).items()})
            write()
            # the backward launches alone
            Lb, c = _lib.lib(), _lib.ctx(dev)
            need = int(Lb.tap_pointer_scores_backward_scratch(B, nR, rows, H))
            need2 = int(Lb.tap_encode_bits_backward_scratch(B, nR, rows, 3 * H))
            scratch = torch.empty(max(need, need2) // 4, device=dev)
            dU, dq = torch.empty(B, 3 * H, nR, device=dev), torch.empty(B, H, device=dev)
            dva, dvp, dM, dk = torch.empty(H, device=dev), torch.empty(H, device=dev), torch.empty(3 * H, rows, device=dev), torch.empty(3 * H, device=dev)
            P = _lib.ptr

            def f_bw1():
                _lib.check(Lb.tap_pointer_scores_backward(c, P(proj), P(bits), B, nR, rows, H, P(Mf), P(k), P(q), P(va), P(vp), P(outs[1]),
                                                          P(outs[2]), P(g), P(dU), P(dq), P(dva), P(dvp), P(scratch), need, _lib.stream_of(dev)), c)

            def f_bw2():
                _lib.check(Lb.tap_encode_bits_backward(c, P(bits), P(dU), B, nR, rows, 3 * H, P(dM), P(dk), P(scratch), need2,
                                                       _lib.stream_of(dev)), c)
            bw = two_runs({"scores_backward": captured(f_bw1, dev, per)[0], "encode_backward_on_dU": captured(f_bw2, dev, per)[0]}, args.reps, per)
            row.update({k2 + "_us": v for k2, v in bw.items()})
            row["dU_bytes"] = dU.numel() * 4
            print(json.dumps(row), flush=True)
            write()
        # the ten-step c2 episode from a hipGraph with the head, both sides on lean steppers
        name, D, n, cs = WINDOWS[0]
        st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
        rows, nR = int(dy.shape[1]), int(dy.shape[2])
        enc = T.DynamicBitsEncoder(rows, H).to(dev)
        sh, dec, hh0 = torch.randn(B, H, nR, device=dev), torch.randn(n, B, H, 1, device=dev), torch.zeros(1, B, H, device=dev)
        graphs, keeps = {}, {}
        with torch.no_grad():
            proj = net.project_static(sh)
            for label in ("forward_bits", "reference"):
                env = T.BatchedContainer(B, cs, n, "C+P+S-lb-soft", "diff", device=dev)
                sp = T.EpisodeStepper(st, dy, env, 'bot', True, steps=n, expand_dynamic=False)
                state = {}

                def scorer(step, sp=sp, state=state, label=label, **_):
                    last = hh0 if step == 0 else state["hh"]
                    if label == "forward_bits":
                        logits, state["hh"] = net.forward_bits(proj, sp.dynamic_bits, enc, dec[step], last)
                    else:
                        logits, state["hh"] = net(sh, enc(sp.dynamic_bits), dec[step], last)
                    return logits
                pol = T.PointerHeadPolicy(scorer, greedy=True)

                def ep(sp=sp, pol=pol):
                    out = T.run_episode(st, dy, pol, cs[0], cs[-1], stepper=sp, check=False)
                    return out["tour_idx"], out["reward"], pol.tour_logp()
                graphs[label], keeps[label] = captured(ep, dev)
            res = two_runs(graphs, args.reps, 1)
        same = float((keeps["forward_bits"][0] == keeps["reference"][0]).float().mean().item())
        episode = {"window": "c2", "B": B, "He": H, "Hd": H, "steps": n, "picks_equal": round(same, 5)}
        episode.update({k2 + "_episode_us": t for k2, t in res.items()})
        print(json.dumps(episode), flush=True)
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    write(episode)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
