#!/usr/bin/env python3
"""Time the 3D actor's decoder step with the height-map encoder inside the launch (heightmap.hip: tap_decoder_step_hm)
against the way a caller had to run it before: ``HeightmapEncoder`` in torch (three strided Conv2d, two leaky_relu), then
``rollout.decoder_step`` with ``identity_dynamic=m``.  The shipped 3D actor's shape -- height map (2, 5, 5), m = 128,
Hd = 256, Ks = 3 -- at BASELINE c3's batch, 4 096; the window for the whole step is c3's (rows 30, nR 60), He = 128 as the
checkpoint has it.

  a_torch_encoder_then_decoder_step    the parent commit's way: encoder(hm), then decoder_step on its (B, m, 1) output
  a_torch_encoder                      its first half alone
  a_decoder_step_kernel                its second half alone, on kept buffers (tap_decoder_step, Kd = m)
  b_decoder_step_heightmap             the new launch through rollout.decoder_step_heightmap
  b_kernel                             the new launch on kept buffers
  c_forward_step_parent                tools.Pointer.forward_step on a fold with identity_dynamic = m, the encoder in torch in front
  c_forward_step_heightmap             tools.Pointer.forward_step on a fold with the HeightmapEncoder: two launches

Clock: device events around a replay of a hipGraph holding ``--per-graph`` calls, after warm-ups; every figure is the
median of ``--reps`` replays, the sides alternating, two runs each.  Writes profiles/heightmap_step.json.  Usage:

    python scripts/time_heightmap_step.py [--reps 30] [--per-graph 4] [--out profiles/heightmap_step.json]
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

B, HE, H, M, KS = 4096, 128, 256, 128, 3
MAP = (2, 5, 5)
WINDOW = ("c3", 3, 10, [5, 5, 50])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--per-graph", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heightmap_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    per = args.per_graph

    def xavier(m):
        for p in m.parameters():
            torch.nn.init.xavier_uniform_(p) if p.dim() > 1 else torch.nn.init.normal_(p, std=0.1)
        return m
    torch.manual_seed(3)
    net = xavier(T.Pointer(HE, H, 'shape_heightmap', 'bot', dropout=0.0)).to(dev).eval()
    name, D, n, cs = WINDOW
    pack.set_binary_check('trust')
    try:
        st, dy = synth.device_rand_instances(B, n, D, seed=7, device=dev)
        rows, nR = int(dy.shape[1]), int(dy.shape[2])
        bits = pack.dynamic_bits(dy)[0]
        enc = T.DynamicBitsEncoder(rows, HE).to(dev)
        dec_s, dec_d = xavier(torch.nn.Conv1d(KS, H - M, 1)).to(dev), xavier(T.HeightmapEncoder(MAP[0], M, MAP[1:])).to(dev)
        sh, hh = torch.randn(B, HE, nR, device=dev), torch.tanh(torch.randn(1, B, H, device=dev))
        ds = torch.randint(1, 6, (B, KS, 1), device=dev).float()
        hm = torch.randint(-50, 51, (B,) + MAP, device=dev).float()
        row = {"window": name, "B": B, "He": HE, "Hd": H, "m": M, "Ks": KS, "map": list(MAP), "rows": rows, "nR": nR}
        with torch.no_grad():
            proj = net.project_static(sh)
            fold_hm = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
            fold_id = net.fold_episode(enc, *net.fold_decoder(dec_s, identity_dynamic=M))
            assert torch.equal(fold_hm.P, fold_id.P) and torch.equal(fold_hm.c, fold_id.c)
            Wq, h2, xs2 = fold_hm.Wq, hh[0], ds.view(B, KS)
            encoded = dec_d(hm).contiguous()
            xd2 = encoded.view(B, M)
            h_out, q_out = torch.empty(B, H, device=dev), torch.empty(B, H, device=dev)
            enc_w = (dec_d.conv1.weight.reshape(M // 4, MAP[0]), dec_d.conv1.bias, dec_d.conv2.weight.reshape(M // 2, M // 4),
                     dec_d.conv2.bias, dec_d.conv3.weight.reshape(M, -1), dec_d.conv3.bias)

            def a_both():
                return rollout.decoder_step(ds, dec_d(hm), h2, fold_id.P, fold_id.c, fold_id.w_hh, fold_id.b_hh, Wq)

            def a_encoder():
                return dec_d(hm)

            def a_kernel():
                rollout._decoder_into(xs2, xd2, h2, fold_id.P, fold_id.c, fold_id.w_hh, fold_id.b_hh, Wq, h_out, q_out, None)

            def b_public():
                return rollout.decoder_step_heightmap(ds, hm, h2, dec_d, fold_hm.P, fold_hm.c, fold_hm.w_hh, fold_hm.b_hh, Wq)

            def b_kernel():
                rollout._decoder_hm_into(xs2, hm, h2, enc_w, fold_hm.P, fold_hm.c, fold_hm.w_hh, fold_hm.b_hh, Wq, h_out, q_out, None, None)

            def c_parent():
                return net.forward_step(proj, bits, fold_id, ds, dec_d(hm), hh)

            def c_new():
                return net.forward_step(proj, bits, fold_hm, ds, hm, hh)
            pa, pb = a_both(), b_public()
            ca, cb = c_parent(), c_new()
            row["max_abs_diff_vs_parent"] = {"h_new": float((pa[0] - pb[0]).abs().max()), "q": float((pa[1] - pb[1]).abs().max()),
                                             "logits": float((ca[0] - cb[0]).abs().max()), "last_hh": float((ca[1] - cb[1]).abs().max())}
            graphs = {k: captured(f, dev, per)[0] for k, f in (
                ("a_torch_encoder_then_decoder_step", a_both), ("a_torch_encoder", a_encoder), ("a_decoder_step_kernel", a_kernel),
                ("b_decoder_step_heightmap", b_public), ("b_kernel", b_kernel), ("c_forward_step_parent", c_parent),
                ("c_forward_step_heightmap", c_new))}
            row.update({k + "_us": v for k, v in two_runs(graphs, args.reps, per).items()})
        pack.check_binary()
    finally:
        pack.set_binary_check('check')
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(dev),
                   "note": "device events around hipGraph replays (%d calls per graph), medians of %d replays after warm-ups, two runs "
                           "each, sides alternating; microseconds" % (per, args.reps),
                   "rows": [row]}, f, indent=1)
    print(json.dumps(row), flush=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
