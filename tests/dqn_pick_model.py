"""Helpers of the one-launch L-Pnet pick's tests (tapenv.h: tap_dqn_pick).

The float64 model is the package's own: ``tools.DQN.double()``, the unfolded torch ops of the reference's forward, and
``rollout.dqn_pick_torch`` on ``net.double().fold()``, the folded algebra of the contract; tests/test_dqn_pick_cpu.py holds
the two together.

Nets: torch.manual_seed(11), DQN(W, diff), the three batch-norms' running statistics drawn as in
tests/test_place_at_cpu.py, head.weight times 8 (seeded heads are near-uniform otherwise), eval().  Inputs: integer
height-maps 0 .. 11 in the net's form (a diff net sees hm[c + 1] - hm[c] and a trailing 0, DRL_L's 'diff'; the other the raw
map), block sides 1 .. 5.

The margin rule is tests/pack_rnn_forward_model.py's: an env is compared on ``x`` only where the float64 model's top-two
PROBABILITY margin is at least MARGIN = 1e-4, and at most CAP = 2 % of a case's envs may be left out.
"""
import numpy as np
import torch

import tap_net_amd as T

MARGIN = 1e-4
CAP = 0.02
# (W, is_diff_height): the reference's W = 5 in both forms (P = 6 / 7 positions, 16 envs per workgroup), the narrowest net
# (P = 3), W = 10 (P = 12) and (9, diff) (P = 10), both 8 envs per workgroup
CASES = [(5, True), (5, False), (2, True), (10, False), (9, True)]


def case_id(c):
    return "w%d-%s" % (c[0], "diff" if c[1] else "full")


def seeded(W, diff, device='cpu', fused=False, dtype=None):
    torch.manual_seed(11)
    net = T.tools.DQN(W, diff, fused=fused)
    for bn in (net.bn1, net.bn2, net.bn3):
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
    with torch.no_grad():
        net.head.weight.mul_(8)
    if dtype is not None:
        net = net.to(dtype)
    return net.to(device).eval()


def inputs(W, diff, B, seed=5):
    """-> height_map (B, 1, W) float32 in the net's form, block (B, 1, 2) float32"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * W + int(diff))
    hm = torch.randint(0, 12, (B, 1, W), generator=g)
    blk = torch.randint(1, 6, (B, 1, 2), generator=g).float()
    if diff:
        hm = torch.cat((hm[:, :, 1:] - hm[:, :, :-1], torch.zeros(B, 1, 1, dtype=hm.dtype)), 2)
    return hm.float(), blk


def margin(probs):
    """the top-two probability margin of every env (float64 probabilities, numpy or torch) -> (B,) numpy"""
    p = np.sort(np.asarray(probs.detach().cpu().numpy() if torch.is_tensor(probs) else probs, np.float64), axis=1)
    return p[:, -1] - p[:, -2]


def compared(probs):
    """the margin rule -> keep (B,) bool; asserts the cap"""
    keep = margin(probs) >= MARGIN
    cut = int((~keep).sum())
    assert cut <= CAP * len(keep), "%d of %d envs under the margin (cap %g)" % (cut, len(keep), CAP)
    return keep
