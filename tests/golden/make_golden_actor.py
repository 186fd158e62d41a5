#!/usr/bin/env python3
"""Generate tests/golden/actor_{2d,3d}_{init,sharp}.npz by running the UPSTREAM REFERENCE's whole actor, model.DRL.forward
(model.py:254-515), on the CPU: 'shape_heightmap', 'bot', rotations allowed, width 5, height 50, 'diff', LB_GREEDY, He = 32,
Hd = 64 (He != Hd: the package's folded_weights slices the two W by He), eval mode, on the first B instances of the committed
dataset_2d.npz (B = 19, 10 blocks, nR 20) / dataset_3d.npz (B = 17, nR 60) -- both cross the decoder kernels' 16-env tile
with a ragged second one.

Two weight sets per dimension, from ONE seeded draw (DRL.__init__'s own: xavier-uniform on every parameter with more than one
axis), float32 and widened exactly for the float64 runs:
  init   the draw as it is: max |logits| 0.1-0.2, the linear part of tanh, a flat softmax;
  sharp  pointer.v and pointer.encoder_attn.v times V_FACTOR, the other pointer.* parameters with more than one axis times
         W_FACTOR: max |logits| in the range the PRETRAINED actor of that dimension has on the same instances (its per-step
         max |logits|, smallest and largest over the steps, is stored as pretrained_logit_range; asserted here: every step
         of 'sharp' lies inside [0.5 x smallest, 2 x largest]).  The checkpoints themselves are too large to commit.

Three runs of the reference's forward per weight set, grad enabled: float64 greedy (its tour_idx is the recorded tour),
float64 with the pick forced to that tour (asserted equal to the greedy run bit for bit) and float32 forced.  A free-running
float32 run cannot be compared: the two rotations of a square block are the same column, the two largest masked logits tie
exactly, and float32 and float64 break the tie differently.  The pick is forced from this side: model.py's module namespace
gets a stand-in for ``torch`` whose ``max`` returns the recorded column and the value at it.  The float64 run's input casts
are forward pre-hooks (the reference feeds float32 height maps).  L = sum_b adv[b] * sum_t tour_logp[b, t], the reference
trainer's actor loss without its mean (trainer.py:222), adv seeded standard normal.

Stored per file: the state dict (sd_<key>, float32), adv, tour_idx, and from the forced float64 run per step the pointer's
output before the mask (logits), last_hh, decoder_static / decoder_dynamic as that step's forward saw them (step 0: zeros),
current_mask; tour_logp, neg_scores, every parameter's gradient of L (grad_<key>, float64); and the float32 run's largest
error against float64: e_ref_logits / e_ref_last_hh per step, e_ref_tour_logp, e_ref_grad_<key> per parameter.  Data only.
One file per weight set: the float64 gradients and the float32 weights of two sets do not fit under the largest committed
fixture (host_reference.npz, 770 887 bytes) together, at any B.  Members carry a fixed time stamp, so the same run gives the
same bytes.  Like make_golden.py it runs only where the reference checkout is present.  Usage:

    python tests/golden/make_golden_actor.py
"""
import copy
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402

HE, HD, N_BLOCKS = 32, 64, 10
BATCH = {2: 19, 3: 17}
SEED = {2: 5200, 3: 5300}
V_FACTOR, W_FACTOR = {2: 300.0, 3: 450.0}, 4.0      # 3D: 300 leaves the last steps below half the pretrained range
SIZE_LIMIT = 770887                  # host_reference.npz, the largest fixture committed before these
WEIGHT_SETS = ("init", "sharp")


def save(path, arrays):
    """np.savez_compressed with a fixed time stamp per member: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asarray(arrays[name]), allow_pickle=False)


class ForcedTorch(object):
    """What model.py sees as ``torch`` during a forced run: everything is torch's, but ``max(probs, 1)`` (model.py:371)
    returns the recorded tour's column of the step and the probability at it"""

    def __init__(self, torch, tour):
        self._torch, self._tour, self.step = torch, tour, 0

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def max(self, probs, dim):
        assert dim == 1 and probs.dim() == 2
        ptr = self._tour[:, self.step].clone()
        self.step += 1
        return probs.gather(1, ptr.unsqueeze(1)).squeeze(1), ptr


def sharpen(torch, actor, D):
    with torch.no_grad():
        for name, p in actor.named_parameters():
            if name in ("pointer.v", "pointer.encoder_attn.v"):
                p.mul_(V_FACTOR[D])
            elif name.startswith("pointer.") and p.dim() > 1:
                p.mul_(W_FACTOR)
    return actor


def run(torch, ref_model, pack, actor, dtype, static, dynamic, adv, forced=None):
    """One forward of the reference's DRL on a copy of ``actor`` in ``dtype`` and one backward of L -> dict of numpy arrays"""
    net = copy.deepcopy(actor).to(dtype).eval()
    D = static.shape[1] - 1
    B = static.shape[0]
    rec = dict(logits=[], last_hh=[], decoder_static=[], decoder_dynamic=[], current_mask=[])

    def msk(mask_, dynamic_, static_, ptr, input_type, allow_rot):
        c, m = pack.update_mask(mask_, dynamic_, static_, ptr, input_type, allow_rot)
        rec["current_mask"].append(c.numpy().astype(np.uint8))
        return c, m

    net.update_fn, net.mask_fn = pack.update_dynamic, msk

    def after_pointer(mod, ins, outs):
        rec["logits"].append(outs[0].detach().double().numpy().copy())
        rec["last_hh"].append(outs[1].detach().double().numpy()[0].copy())

    def before_static_decoder(mod, ins):
        rec["decoder_static"].append(ins[0].detach().numpy().copy())

    def before_dynamic_decoder(mod, ins):
        rec["decoder_dynamic"].append(ins[0].detach().numpy().copy())
        return (ins[0].to(dtype),)      # the reference hands it torch.FloatTensor(heightmaps) whatever the model's dtype is

    hooks = [net.pointer.register_forward_hook(after_pointer),
             net.static_decoder.register_forward_pre_hook(before_static_decoder),
             net.dynamic_decoder.register_forward_pre_hook(before_dynamic_decoder)]
    n = N_BLOCKS
    move = dynamic[:, :n].sum(1); small = dynamic[:, n:2 * n].sum(1); large = dynamic[:, 2 * n:].sum(1)
    cur = torch.ones(B, static.shape[2])
    cur[(small * large + move).ne(0)] = 0.                      # model.py:297-307: the mask step 0 sees
    rec["current_mask"].append(cur.numpy().astype(np.uint8))
    dec = [torch.zeros(B, D, 1, dtype=dtype), torch.zeros(B, 4, 1, dtype=dtype) if D == 2 else torch.zeros(B, 2, 5, 5, dtype=dtype)]
    real = ref_model.torch
    stand_in = ForcedTorch(real, forced) if forced is not None else None
    try:
        if stand_in is not None:
            ref_model.torch = stand_in
        with torch.enable_grad():
            tour_idx, tour_logp, _, neg_scores = net(static.to(dtype), dynamic.to(dtype), dec)
    finally:
        ref_model.torch = real
        for h in hooks:
            h.remove()
    steps = tour_idx.shape[1]
    assert steps == n and len(rec["logits"]) == n and (stand_in is None or stand_in.step == n)
    (adv.to(dtype) * tour_logp.sum(1)).sum().backward()
    out = {k: np.stack(v[:n]) for k, v in rec.items()}           # (the mask after the last step is not one a step saw)
    out.update(tour_idx=tour_idx.numpy(), tour_logp=tour_logp.detach().double().numpy(), neg_scores=neg_scores.numpy(),
               grads={k: p.grad.detach().double().numpy() for k, p in net.named_parameters()})
    return out


def pretrained_range(torch, ref_model, pack, D, static, dynamic):
    """the pretrained actor of dimension D on the same instances, greedy, as the reference runs it (float32): the smallest
    and the largest per-step max |logits|"""
    actor = ref_model.DRL(D, 3 * N_BLOCKS, 128, 256, False, "bot", True, 5, 50, D, "C+P+S-lb-soft",
                          "shape_heightmap", "diff", "LB_GREEDY", pack.update_dynamic, pack.update_mask, 1, 0.1, 1.0)
    ck = os.path.join(ref_loader.REFERENCE_DIR, "pretrain_model", "%dd-bot-C+P+S-lb-soft-width-5-note-sh-R-diff" % D, "actor.pt")
    actor.load_state_dict(torch.load(ck, map_location="cpu"))
    actor.eval()
    peaks = []
    h = actor.pointer.register_forward_hook(lambda mod, ins, out: peaks.append(float(out[0].abs().max())))
    B = static.shape[0]
    with torch.no_grad():
        actor(static, dynamic, [torch.zeros(B, D, 1), torch.zeros(B, 4, 1) if D == 2 else torch.zeros(B, 2, 5, 5)])
    h.remove()
    assert len(peaks) == N_BLOCKS
    return np.array([min(peaks), max(peaks)], np.float64)


def main():
    mods = ref_loader.load()
    if mods is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    _, pack, _ = mods
    import torch
    torch.set_num_threads(1)
    sys.path.insert(0, ref_loader.REFERENCE_DIR)
    try:
        import model as ref_model
    finally:
        sys.path.remove(ref_loader.REFERENCE_DIR)
    for D in (2, 3):
        B = BATCH[D]
        ds = np.load(os.path.join(HERE, "dataset_%dd.npz" % D))
        static = torch.from_numpy(ds["static"][:B].astype(np.float32))
        dynamic = torch.from_numpy(ds["dynamic"][:B].astype(np.float32))
        assert static.shape[0] == B and B > 16 and B % 16 and static.shape[2] == N_BLOCKS * (2 if D == 2 else 6)
        rng_range = pretrained_range(torch, ref_model, pack, D, static, dynamic)
        torch.manual_seed(SEED[D])
        base = ref_model.DRL(D, 3 * N_BLOCKS, HE, HD, False, "bot", True, 5, 50, D, "C+P+S-lb-soft",
                             "shape_heightmap", "diff", "LB_GREEDY", pack.update_dynamic, pack.update_mask, 1, 0.1, 1.0).eval()
        adv = torch.randn(B, generator=torch.Generator().manual_seed(SEED[D] + 1))
        for ws in WEIGHT_SETS:
            actor = sharpen(torch, copy.deepcopy(base), D) if ws == "sharp" else base
            greedy = run(torch, ref_model, pack, actor, torch.float64, static, dynamic, adv)
            tour = torch.from_numpy(greedy["tour_idx"])
            f64 = run(torch, ref_model, pack, actor, torch.float64, static, dynamic, adv, forced=tour)
            f32 = run(torch, ref_model, pack, actor, torch.float32, static, dynamic, adv, forced=tour)
            assert np.array_equal(f64["tour_idx"], greedy["tour_idx"]) and np.array_equal(f32["tour_idx"], greedy["tour_idx"])
            for k in greedy:                                     # the forced float64 run IS the greedy one
                if k == "grads":
                    assert all(np.array_equal(greedy[k][p], f64[k][p]) for p in greedy[k]), k
                else:
                    assert np.array_equal(greedy[k], f64[k]), k
            peaks = np.abs(f64["logits"]).max(axis=(1, 2))
            print("%dD %s: per-step max |logits| %.4g .. %.4g; pretrained %.4g .. %.4g" % (D, ws, peaks.min(), peaks.max(), *rng_range))
            if ws == "sharp":
                assert (peaks >= 0.5 * rng_range[0]).all() and (peaks <= 2.0 * rng_range[1]).all(), (peaks, rng_range)
            out = dict(adv=adv.numpy(), tour_idx=f64["tour_idx"].astype(np.int16), logits=f64["logits"], last_hh=f64["last_hh"],
                       decoder_static=f64["decoder_static"].astype(np.int16), decoder_dynamic=f64["decoder_dynamic"].astype(np.int16),
                       current_mask=f64["current_mask"], tour_logp=f64["tour_logp"], neg_scores=f64["neg_scores"].astype(np.float32),
                       pretrained_logit_range=rng_range, sharp_factors=np.array([V_FACTOR[D], W_FACTOR]),
                       e_ref_logits=np.abs(f32["logits"] - f64["logits"]).max(axis=(1, 2)),
                       e_ref_last_hh=np.abs(f32["last_hh"] - f64["last_hh"]).max(axis=(1, 2)),
                       e_ref_tour_logp=np.abs(f32["tour_logp"] - f64["tour_logp"]).max())
            for name in ("decoder_static", "decoder_dynamic"):   # integers: int16 holds them exactly
                assert np.array_equal(out[name].astype(np.float64), f64[name].astype(np.float64)), name
            assert np.array_equal(out["neg_scores"], f64["neg_scores"])
            for k, v in actor.state_dict().items():
                out["sd_" + k] = v.numpy().astype(np.float32)
                assert np.array_equal(out["sd_" + k], v.numpy())
                out["grad_" + k] = f64["grads"][k]
                out["e_ref_grad_" + k] = np.abs(f32["grads"][k] - f64["grads"][k]).max()
                assert np.abs(f64["grads"][k]).max() > 0, k
            print("  e_ref: logits %.3g  last_hh %.3g  tour_logp %.3g  gradients (relative to each one's largest) %.3g" % (
                out["e_ref_logits"].max(), out["e_ref_last_hh"].max(), out["e_ref_tour_logp"],
                max(out["e_ref_grad_" + k] / np.abs(out["grad_" + k]).max() for k in f64["grads"])))
            path = os.path.join(HERE, "actor_%dd_%s.npz" % (D, ws))
            save(path, out)
            size = os.path.getsize(path)
            print("  wrote %s (%d bytes)" % (path, size))
            assert size < SIZE_LIMIT, size


if __name__ == "__main__":
    main()
