#!/usr/bin/env python3
"""Generate tests/golden/dqn_pick.npz by running the UPSTREAM REFERENCE's tools.DQN in eval mode on the recipe of
tests/dqn_pick_model.py, for the cases the reference can build (its lin1 is sized for W = 5 only: both input forms there):
per case (W, is_diff_height) the float32 probabilities of 64 inputs, the inputs themselves, the
parameter names and shapes, and ``err``, the reference's own float32 error -- the largest difference between those
probabilities and the same reference network's in float64.  The weights are too large for a fixture: the test rebuilds them
from the same seed (same layers, same construction order), as place_at.npz does.  It runs only where the reference checkout
is present.  Usage:

    python tests/golden/make_golden_dqn_pick.py
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the package, for dqn_pick_model's inputs
import ref_loader  # noqa: E402
import dqn_pick_model as DM  # noqa: E402

N = 64
REF_CASES = [c for c in DM.CASES if c[0] == 5]


def main():
    mods = ref_loader.load()
    if mods is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    tools = mods[0]
    import torch
    out = {}
    for W, diff in REF_CASES:
        torch.manual_seed(11)
        net = tools.DQN(W, diff)
        for bn in (net.bn1, net.bn2, net.bn3):
            bn.running_mean.uniform_(-0.5, 0.5)
            bn.running_var.uniform_(0.5, 2.0)
        with torch.no_grad():
            net.head.weight.mul_(8)
        net.eval()
        hm, blk = DM.inputs(W, diff, N)
        with torch.no_grad():
            y = net(hm, blk)
            y64 = copy.deepcopy(net).double()(hm.double(), blk.double())
        key = DM.case_id((W, diff))
        sd = net.state_dict()
        out[key + "_sd_keys"] = np.asarray(list(sd))
        out[key + "_sd_shapes"] = np.asarray([",".join(str(d) for d in v.shape) for v in sd.values()])
        out[key + "_hm"] = hm.numpy()
        out[key + "_block"] = blk.numpy()
        out[key + "_out"] = y.numpy()
        out[key + "_err"] = np.float64((y.double() - y64).abs().max().item())
    out["cases"] = np.asarray([DM.case_id(c) for c in REF_CASES])
    np.savez_compressed(os.path.join(HERE, "dqn_pick.npz"), **out)


if __name__ == "__main__":
    main()
