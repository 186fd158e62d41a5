#!/usr/bin/env python3
"""Time the state critic on the bit shadow (critic.hip: tap_critic_value, one launch) against the module's torch path,
which is the reference's arithmetic (trainer.py:18-94).  B = 8 192, H = 128, three process blocks, windows (rows, nR) =
(30, 20) [c2] and (30, 60) [c3]; the instances' own shadow and static input (static[:, 1:1 + D]); the trainer's zero x0
(decoder_input=None).  Forward, under no_grad:

  value_kernel       the launch alone on kept buffers
  module_shadow      tools.StateCritic.forward on the int64 shadow: the one-row GRU step, fold(), the launch
  module_torch       tools.StateCritic.forward on the fp32 `dynamic`: the reference's Conv1d, concatenations and bmm

Forward + backward (gradients of every parameter of sum_b a[b] est[b]): ``critic_value`` under autograd from its folded
leaves (the three backward launches and the batch sums), the module on the shadow and the module's torch path under torch
autograd; and the backward launches alone (tap_critic_value_backward, tap_encode_bits_backward on dU).

Clock: device events around a replay of a hipGraph holding ``--per-graph`` calls, after warm-ups; every figure is the
median of ``--reps`` replays, the sides alternating, two runs each.  No speed bar: the numbers are recorded as they come
out.  ``--window`` runs one window (a process of its own per window, so each can stand under its own time limit); the
rows of the other windows already in the file are kept.  Usage:

    python scripts/time_critic.py [--window c2] [--reps 30] [--per-graph 4] [--out profiles/critic.json]
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

B, H, BLOCKS = 8192, 128, 3
WINDOWS = {"c2": (2, 10), "c3": (3, 10)}
EPISODE_US = 1560.0     # the ten-step c2 episode with the head (DESIGN 7i / INTEGRATION 2i), for the critic's share of an iteration


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", choices=sorted(WINDOWS), action="append")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--per-graph", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "critic.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    per = args.per_graph
    rows_out = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            rows_out = [r for r in json.load(f).get("rows", []) if r["window"] not in (args.window or sorted(WINDOWS))]

    def write():
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev),
                       "note": "device events around hipGraph replays (%d calls per graph), medians of %d replays after warm-ups, "
                               "two runs each, sides alternating; microseconds" % (per, args.reps),
                       "rows": sorted(rows_out, key=lambda r: r["window"])}, f, indent=1)

    pack.set_binary_check('trust')
    try:
        for name in args.window or sorted(WINDOWS):
            D, n = WINDOWS[name]
            st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
            rows, nR = int(dy.shape[1]), int(dy.shape[2])
            x = st[:, 1:1 + D, :].contiguous()
            bits = pack.dynamic_bits(dy)[0]
            torch.manual_seed(3)
            net = T.StateCritic(D, rows, H, n_process_blocks=BLOCKS).to(dev)
            for p in net.parameters():
                if p.dim() > 1:
                    torch.nn.init.xavier_uniform_(p)
            a = torch.randn(B, device=dev)
            row = {"window": name, "B": B, "H": H, "S": D, "blocks": BLOCKS, "rows": rows, "nR": nR,
                   "static_bytes": x.numel() * 4, "shadow_bytes": bits.numel() * 8, "ones_share": round(float(dy.mean().item()), 4),
                   "reference_concat_bytes_per_block": B * 3 * H * nR * 4, "dynamic_hidden_bytes": B * H * nR * 4,
                   "tanhf_per_call": B * BLOCKS * nR * H}
            rows_out.append(row)
            net.eval()
            with torch.no_grad():
                f = net.fold()
                leaves = [t.detach().contiguous() for t in (f.G, f.g, f.M, net._rnn_out(x, None, None).matmul(f.Wq.t()), f.v, f.w2, f.b2)]
                outs = rollout._critic_buffers(B, D, nR, H, BLOCKS, dev)
                f_kernel = lambda: rollout._critic_into(x, bits, *leaves, BLOCKS, rows, *outs)            # noqa: E731
                f_shadow = lambda: net(x, bits)                                                          # noqa: E731
                f_torch = lambda: net(x, dy)                                                             # noqa: E731
                row["max_abs_diff_vs_torch_path"] = float((f_shadow() - f_torch()).abs().max())
                graphs = {"value_kernel": captured(f_kernel, dev, per)[0], "module_shadow": captured(f_shadow, dev, per)[0],
                          "module_torch": captured(f_torch, dev, per)[0]}
                row.update({k + "_us": v for k, v in two_runs(graphs, args.reps, per).items()})
            row["tanhf_per_ns"] = round(row["tanhf_per_call"] / (min(row["value_kernel_us"]) * 1e3), 2)
            write()
            # forward + backward
            net.train()
            L1 = [t.clone().requires_grad_(True) for t in leaves]
            params = list(net.parameters())
            fb = {"critic_value": lambda: torch.autograd.grad((T.critic_value(x, bits, *L1, BLOCKS, rows=rows) * a).sum(), L1),
                  "module_shadow": lambda: torch.autograd.grad((net(x, bits).view(-1) * a).sum(), params),
                  "module_torch": lambda: torch.autograd.grad((net(x, dy).view(-1) * a).sum(), params)}
            graphs = {}
            for label, fn in fb.items():
                try:
                    graphs[label] = captured(fn, dev, per)[0]
                except RuntimeError as e:                                                                # a side that does not capture is recorded as such
                    row["fwd_bwd_" + label + "_error"] = str(e).splitlines()[0][:200]
                    torch.cuda.synchronize()
            row.update({"fwd_bwd_" + k + "_us": v for k, v in two_runs(graphs, args.reps, per).items()})
            write()
            # the backward launches alone
            Lb, c, P = _lib.lib(), _lib.ctx(dev), _lib.ptr
            need = int(Lb.tap_critic_value_backward_scratch(B, nR, rows, H, D, BLOCKS))
            need2 = int(Lb.tap_encode_bits_backward_scratch(B, nR, rows, H))
            scratch = torch.empty(max(need, need2) // 4, device=dev)
            dz, dU, dq = torch.randn(B, H, device=dev), torch.empty(B, H, nR, device=dev), torch.empty(B, BLOCKS, H, device=dev)
            dv, dM, dk = torch.empty(H, device=dev), torch.empty(H, rows, device=dev), torch.empty(H, device=dev)
            G, g, Mf, _, v = leaves[:5]

            def f_bw1():
                _lib.check(Lb.tap_critic_value_backward(c, P(x), P(bits), B, nR, rows, H, D, BLOCKS, P(G), P(g), P(Mf), P(v), P(outs[4]),
                                                        P(outs[2]), P(dz), P(dU), P(dq), P(dv), P(scratch), need, _lib.stream_of(dev)), c)

            def f_bw2():
                _lib.check(Lb.tap_encode_bits_backward(c, P(bits), P(dU), B, nR, rows, H, P(dM), P(dk), P(scratch), need2,
                                                       _lib.stream_of(dev)), c)
            bw = two_runs({"value_backward": captured(f_bw1, dev, per)[0], "encode_backward_on_dU": captured(f_bw2, dev, per)[0]}, args.reps, per)
            row.update({k + "_us": v for k, v in bw.items()})
            row["dU_bytes"] = dU.numel() * 4
            if name == "c2":
                row["episode_us_recorded"] = EPISODE_US
                for k in ("module_shadow", "module_torch"):
                    if "fwd_bwd_" + k + "_us" in row:
                        t = min(row["fwd_bwd_" + k + "_us"])
                        row["share_of_iteration_" + k] = round(t / (EPISODE_US + t), 4)
            print(json.dumps(row), flush=True)
            write()
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    print("wrote", args.out)


if __name__ == "__main__":
    main()
