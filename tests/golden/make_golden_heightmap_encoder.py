#!/usr/bin/env python3
"""Generate tests/golden/heightmap_encoder.npz by running the UPSTREAM REFERENCE's HeightmapEncoder (model.py:21-35) on the
CPU in float64:

  * ``pre_<key>``: every ``dynamic_decoder.*`` tensor of the shipped 3D actor
    (pretrain_model/3d-bot-C+P+S-lb-soft-width-5-note-sh-R-diff/actor.pt), float32 as stored;
  * ``pre_out`` (640, 128) float64: the reference module holding those tensors on the 640 height maps that
    tests/golden/episode_3d.npz records (``features`` (10, 64, 50) viewed as (640, 2, 5, 5));
  * for (C, hidden, W, L) in CASES: a seeded xavier-uniform state dict ``c<i>_sd_<key>`` (float32), three inputs ``c<i>_x``
    (3, C, W, L) -- integers in [-50, 50], drawn in float32 -- and the module's float64 outputs ``c<i>_out`` (3, hidden).

Parameters and inputs are float32 values widened to float64 for the run, so the fixture stores them without loss.  Data
only.  Like make_golden_pointer.py it runs only where the reference checkout is present.  Usage:

    python tests/golden/make_golden_heightmap_encoder.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402

CASES = [(1, 64, 5, 5), (4, 64, 5, 5), (2, 64, 10, 10), (1, 32, 4, 12), (2, 32, 5, 6)]
ACTOR = os.path.join("pretrain_model", "3d-bot-C+P+S-lb-soft-width-5-note-sh-R-diff", "actor.pt")
PREFIX = "dynamic_decoder."


def main():
    if ref_loader.load() is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    import torch
    sys.path.insert(0, ref_loader.REFERENCE_DIR)
    try:
        import model as ref_model
    finally:
        sys.path.remove(ref_loader.REFERENCE_DIR)
    out = {"cases": np.array(["%d,%d,%d,%d" % c for c in CASES])}
    # the shipped 3D actor's encoder on the recorded episode's height maps
    sd = torch.load(os.path.join(ref_loader.REFERENCE_DIR, ACTOR), map_location="cpu")
    sd = {k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX)}
    net = ref_model.HeightmapEncoder(2, 128, (5, 5))
    net.load_state_dict(sd, strict=True)
    for k, v in sd.items():
        assert v.dtype == torch.float32
        out["pre_" + k] = v.numpy()
    feats = np.load(os.path.join(HERE, "episode_3d.npz"))["features"]
    assert feats.shape == (10, 64, 50)
    x = torch.from_numpy(feats.reshape(640, 2, 5, 5).astype(np.float64))
    with torch.no_grad():
        out["pre_out"] = net.double()(x).squeeze(-1).numpy()
    assert out["pre_out"].shape == (640, 128) and out["pre_out"].dtype == np.float64
    # seeded modules of the other shapes
    for i, (C, hidden, W, L) in enumerate(CASES):
        torch.manual_seed(4200 + i)
        net = ref_model.HeightmapEncoder(C, hidden, (W, L))
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
        x = torch.randint(-50, 51, (3, C, W, L)).float()
        pre = "c%d_" % i
        for k, v in net.state_dict().items():
            out[pre + "sd_" + k] = v.numpy().copy()
        net = net.double()
        with torch.no_grad():
            y = net(x.double()).squeeze(-1)
        out[pre + "x"] = x.numpy()
        out[pre + "out"] = y.numpy()
        assert out[pre + "out"].shape == (3, hidden) and out[pre + "out"].dtype == np.float64
    path = os.path.join(HERE, "heightmap_encoder.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
