#!/usr/bin/env python3
"""Generate tests/golden/pointer.npz by running the UPSTREAM REFERENCE's Pointer (model.py:77-138; its Attention,
model.py:38-74) on the CPU in float64, eval mode: for (He, Hd) = (32, 32) and (16, 32), B = 3, nR = 8, seeded
xavier-uniform parameters (the reference's own initialisation of every parameter with more than one axis) -- the state
dict, the four inputs (static_hidden, dynamic_hidden, decoder_hidden, last_hh), and the outputs probs and last_hh.
Parameters and inputs are drawn in float32 and widened, so the fixture stores them as float32 without loss; the outputs
are float64.  No kernel exists for Hd = 32, so these cases reach the package's torch path only; the kernel path is pinned to
the reference by make_golden_actor.py's fixtures (the whole DRL at He = 32, Hd = 64).  Data only.  Like make_golden.py it runs only where the reference checkout is present.  Usage:

    python tests/golden/make_golden_pointer.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402

CASES = [(32, 32), (16, 32)]
B, NR = 3, 8


def main():
    if ref_loader.load() is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    import torch
    sys.path.insert(0, ref_loader.REFERENCE_DIR)
    try:
        import model as ref_model
    finally:
        sys.path.remove(ref_loader.REFERENCE_DIR)
    out = {"cases": np.array(["%d,%d" % c for c in CASES])}
    for i, (He, Hd) in enumerate(CASES):
        torch.manual_seed(4100 + i)
        net = ref_model.Pointer(He, Hd, 'shape_heightmap', 'bot')
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)
        net = net.double().eval()
        ins = (torch.randn(B, He, NR).double(), torch.randn(B, He, NR).double(), torch.randn(B, Hd, 1).double(),
               torch.randn(1, B, Hd).double())
        with torch.no_grad():
            probs, last_hh = net(*ins)
        pre = "c%d_" % i
        for k, v in net.state_dict().items():
            out[pre + "sd_" + k] = v.numpy().astype(np.float32)
            assert np.array_equal(out[pre + "sd_" + k].astype(np.float64), v.numpy())
        for name, v in zip(("static_hidden", "dynamic_hidden", "decoder_hidden", "last_hh_in", "probs", "last_hh"),
                           ins + (probs, last_hh)):
            a = v.numpy()
            out[pre + name] = a if name in ("probs", "last_hh") else a.astype(np.float32)
            assert np.array_equal(out[pre + name].astype(np.float64), a)
    path = os.path.join(HERE, "pointer.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
