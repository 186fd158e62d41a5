#!/usr/bin/env python3
"""Generate tests/golden/critic_{2d,3d}_{xavier,sharp}.npz by running the UPSTREAM REFERENCE's critic, trainer.realCritic
(trainer.py:44-94), on the CPU as its trainer calls it (trainer.py:205-214): input type 'bot', so static_input =
encoder_static[:, 1:1 + obj_dim, :], the initial ``dynamic`` and the zero x0; H = 64, three process blocks, eval mode, on
the first B instances of the committed dataset_2d.npz (B = 19, nR 20) / dataset_3d.npz (B = 17, nR 60).

As constructed the critic's attention.v and attention.W are zeros: the softmax is uniform and tests nothing.  Two weight
sets per dimension, from ONE seeded draw, float32 and widened exactly for the float64 runs:
  xavier  xavier-uniform on every parameter with more than one axis;
  sharp   attention.v times the smallest power of 2^(1/2) for which the spread max_c s - min_c s of the attention's
          logits is at least 1 for every env and block: every softmax then has a largest-to-smallest ratio of e or more,
          and the largest spreads are 3.7 (2D) and 1.9 (3D).
The PRETRAINED critics cannot calibrate 'sharp': in all four checkpoints attention.v and attention.W are exactly zero (as
constructed they are zeros, and with both zero neither ever receives a gradient), so the spread the pretrained critic of
either dimension shows on these instances is 0 .. 0.  That finding is recorded as pretrained_s_spread = [smallest, largest]
and asserted here to be [0, 0]; the checkpoints themselves are not committed.

Stored per file (float64 unless named): the state dict (sd_<key>, float32), static_input, dynamic, the seeded weights a of
L = sum_b a[b] est[b], est (B,), p (B, 3, nR) the attention's output per block, s_spread (B, 3), every parameter's gradient
of L (grad_<key>), the float32 run's largest error against float64 (e_ref_est, e_ref_p, e_ref_grad_<key>),
pretrained_s_spread, sharp_factor, and pretrained_keys: 'checkpoint directory|key|shape' of the four pretrained critic.pt
(names and shapes only).  Data only.  Members carry a fixed time stamp, so the same run gives the same bytes.  Like
make_golden.py it runs only where the reference checkout is present.  Usage:

    python tests/golden/make_golden_critic.py
"""
import copy
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
from make_golden_actor import save  # noqa: E402

H, BLOCKS = 64, 3
BATCH = {2: 19, 3: 17}
SEED = {2: 6200, 3: 6300}
WEIGHT_SETS = ("xavier", "sharp")
SHARP_SPREAD = 1.0
PRETRAINED = "%dd-bot-C+P+S-lb-soft-width-5-note-sh-%s-diff"


def run(torch, critic, dtype, static, dynamic, a):
    """one forward of the reference's critic on a copy of ``critic`` in ``dtype`` and one backward of L -> dict"""
    net = copy.deepcopy(critic).to(dtype).eval()
    ps, spreads = [], []

    def watch(mod, ins, out):
        ps.append(out.detach().double().squeeze(1).numpy().copy())
        sh, dh, dec = (t.detach() for t in ins)
        hidden = torch.cat((sh, dh, dec.unsqueeze(2).expand_as(sh)), 1)
        s = torch.matmul(mod.v[0].detach(), torch.tanh(torch.matmul(mod.W[0].detach(), hidden))).squeeze(1)
        spreads.append((s.max(1)[0] - s.min(1)[0]).double().numpy())
    h = net.attention.register_forward_hook(watch)
    x0 = torch.zeros_like(static[:, :, 0]).unsqueeze(2).to(dtype)                  # trainer.py:213
    with torch.enable_grad():
        est = net(static.to(dtype), dynamic.to(dtype), x0).view(-1)
        (a.to(dtype) * est).sum().backward()
    h.remove()
    return dict(est=est.detach().double().numpy(), p=np.stack(ps, 1), s_spread=np.stack(spreads, 1),
                grads={k: v.grad.detach().double().numpy() for k, v in net.named_parameters()})


def pretrained(torch, ref_trainer, D, static, dynamic):
    """the pretrained critic of dimension D on the same instances -> [smallest, largest] spread; and the key list of both
    of that dimension's checkpoints"""
    keys, rng = [], None
    for tag in ("G", "R"):
        name = PRETRAINED % (D, tag)
        sd = torch.load(os.path.join(ref_loader.REFERENCE_DIR, "pretrain_model", name, "critic.pt"), map_location="cpu")
        keys += ["%s|%s|%s" % (name, k, "x".join(str(d) for d in v.shape)) for k, v in sd.items()]
        if tag == "R":
            hid = int(sd["attention.v"].shape[2])
            net = ref_trainer.realCritic(int(sd["static_encoder.conv.weight"].shape[1]), int(sd["dynamic_encoder.conv.weight"].shape[1]),
                                         hid, 1, BLOCKS, 0.1)
            net.load_state_dict(sd, strict=True)
            out = run(torch, net, torch.float32, static, dynamic, torch.ones(static.shape[0]))
            rng = np.array([out["s_spread"].min(), out["s_spread"].max()], np.float64)
    return rng, keys


def main():
    if ref_loader.load() is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    import torch
    torch.set_num_threads(1)
    sys.path.insert(0, ref_loader.REFERENCE_DIR)
    try:
        import trainer as ref_trainer
    finally:
        sys.path.remove(ref_loader.REFERENCE_DIR)
    limit = max(os.path.getsize(f) for f in glob.glob(os.path.join(HERE, "actor_*.npz")))
    for D in (2, 3):
        B = BATCH[D]
        ds = np.load(os.path.join(HERE, "dataset_%dd.npz" % D))
        static = torch.from_numpy(ds["static"][:B, 1:1 + D, :].astype(np.float32))            # trainer.py:211
        dynamic = torch.from_numpy(ds["dynamic"][:B].astype(np.float32))
        assert set(np.unique(dynamic.numpy())) <= {0.0, 1.0}
        rng_range, keys = pretrained(torch, ref_trainer, D, static, dynamic)
        assert rng_range[0] == 0.0 and rng_range[1] == 0.0, rng_range               # (see the docstring)
        torch.manual_seed(SEED[D])
        base = ref_trainer.realCritic(D, int(dynamic.shape[1]), H, 1, BLOCKS, 0.1).eval()
        for p in base.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
        a = torch.randn(B, generator=torch.Generator().manual_seed(SEED[D] + 1))
        for ws in WEIGHT_SETS:
            factor = 1.0
            while True:
                critic = copy.deepcopy(base)
                with torch.no_grad():
                    critic.attention.v.mul_(factor)
                f64 = run(torch, critic, torch.float64, static, dynamic, a)
                sp = f64["s_spread"]
                if ws == "xavier" or sp.min() >= SHARP_SPREAD:
                    break
                assert factor < 2.0 ** 20, (factor, sp.min(), sp.max())
                factor *= 2.0 ** 0.5
            f32 = run(torch, critic, torch.float32, static, dynamic, a)
            print("%dD %s: v x %.4g, spread %.4g .. %.4g; pretrained %.4g .. %.4g; est %.4g .. %.4g" % (
                D, ws, factor, sp.min(), sp.max(), *rng_range, f64["est"].min(), f64["est"].max()))
            assert sp.min() > 0 and (ws == "xavier" or sp.min() >= SHARP_SPREAD)
            out = dict(static_input=static.double().numpy(), dynamic=dynamic.double().numpy(), a=a.double().numpy(),
                       est=f64["est"], p=f64["p"], s_spread=sp, pretrained_s_spread=rng_range, sharp_factor=np.float64(factor),
                       pretrained_keys=np.array(keys), e_ref_est=np.abs(f32["est"] - f64["est"]).max(),
                       e_ref_p=np.abs(f32["p"] - f64["p"]).max())
            for k, v in critic.state_dict().items():
                out["sd_" + k] = v.numpy().astype(np.float32)
                assert np.array_equal(out["sd_" + k], v.numpy())
                out["grad_" + k] = f64["grads"][k]
                out["e_ref_grad_" + k] = np.abs(f32["grads"][k] - f64["grads"][k]).max()
            zero = [k for k in f64["grads"] if not np.abs(f64["grads"][k]).max() > 0]
            print("  e_ref: est %.3g  p %.3g  gradients (relative to each one's largest) %.3g; all-zero gradients: %s" % (
                out["e_ref_est"], out["e_ref_p"],
                max(out["e_ref_grad_" + k] / max(np.abs(out["grad_" + k]).max(), 1e-300) for k in f64["grads"]), zero))
            path = os.path.join(HERE, "critic_%dd_%s.npz" % (D, ws))
            save(path, out)
            size = os.path.getsize(path)
            print("  wrote %s (%d bytes)" % (path, size))
            assert size <= limit, (size, limit)


if __name__ == "__main__":
    main()
