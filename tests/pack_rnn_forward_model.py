"""Helpers of the one-launch PackRNN forward's tests (tapenv.h: tap_pack_rnn_forward).

The float64 model is the package's own: ``tools.PackRNN.double()`` on the numpy engine (tests/pack_engine_model.py), the
unfolded torch ops of the reference's forward, and ``rollout.pack_rnn_forward_torch`` in float64, the folded algebra of
the contract; tests/test_pack_rnn_forward_cpu.py holds the two together.

Nets are seeded as tests/test_pack_rnn_gpu.py: _seeded builds them.  Xavier weights give near-uniform columns (the
fixture's top-two margins are 1e-5 .. 1e-3), so the nets are sharpened: fc.2.weight times 16, fc.0.weight times 2.

The margin rule: an env is compared up to, not including, the first step at which the float64 model's top-two
PROBABILITY margin is below MARGIN = 1e-4 (the fixture's threshold) -- a float32 forward may pick the other column there,
and everything after it differs.  The cap: at most CAP = 2 % of a case's envs may be cut short this way; the tests
assert it, so a comparison never goes vacuous.
"""
import copy

import numpy as np
import torch

import pack_engine_model as M
import tap_net_amd as T

H = 60
MARGIN = 1e-4
CAP = 0.02
TILE = 16       # envs per workgroup of k_pack_rnn_forward (the launch record's third field)
# test 1 of tests/test_pack_rnn_forward_gpu.py: (kind, W, heightmap_type, blocks_num, T, B, seed of the blocks).  W 2 / 5 /
# 10 / 64 (one / three 32-term blocks of the height product, W' = 1), the three types spread over them; (1, 1) no hidden
# product, (10, 10) / (20, 20) a clear exactly at the end, (12, 12) / (20, 20) wraps mid-forward, (7, 12) an encoder longer
# than the decoder; B 1, 5, a tile, a tile + 1, 130 (nine workgroups, the last with two envs).
CASES = [('G', 2, 'full', 1, 1, 1, 7), ('G', 5, 'diff', 7, 7, 5, 7), ('LG', 5, 'diff', 10, 10, TILE, 7),
         ('G', 10, 'zero', 12, 12, TILE + 1, 8), ('LG', 10, 'full', 20, 20, 130, 7), ('G', 64, 'diff', 7, 12, 130, 7),
         ('LG', 64, 'zero', 12, 12, 130, 7), ('LG', 2, 'diff', 7, 12, TILE + 1, 7), ('G', 5, 'diff', 20, 20, 130, 7),
         ('G', 64, 'full', 10, 10, 5, 7)]


def case_id(c):
    return "%s-w%d-%s-n%d-t%d-b%d" % c[:6]


def case_net(c, device='cpu', fused=False):
    kind, W, t = c[:3]
    return sharpen(seeded(kind, W, seed=3, heightmap_type=t, device=device, fused=fused))


def seeded(kind, W, seed=None, heightmap_type='diff', engine=None, device='cpu', fused=False, height=H, max_blocks_num=10):
    torch.manual_seed(1000 + 10 * W + (1 if kind == 'LG' else 0) if seed is None else seed)
    net = T.tools.PackRNN(2, 128, W, 128, W, height, heightmap_type, max_blocks_num=max_blocks_num, pack_net_type=kind,
                          engine=(M.factory() if str(device) == 'cpu' else None) if engine is None else engine, fused=fused)
    return net.to(device).eval()


def sharpen(net):
    with torch.no_grad():
        net.fc[2].weight.mul_(16)
        net.fc[0].weight.mul_(2)
    return net


def host_copy(net, dtype):
    """the same weights on the host in ``dtype``, on the numpy engine, unfused"""
    c = copy.deepcopy(net).to('cpu').to(dtype)
    c.fused, c.engine_factory, c._engine, c._fold = False, M.factory(), None, None
    c.captured_engines = []
    return c.eval()


def make_blocks(B, T_, W, seed, wide=0.0, hmax=4):
    """(B, 2, T) float32: widths 1 .. W, heights 1 .. hmax, 20 % of the sides with a fractional part (the net reads it,
    the engine truncates it); a share ``wide`` of the widths is W + 1 (error bit 4)"""
    rs = np.random.RandomState(seed)
    w = rs.randint(1, W + 1, (B, T_)) + (rs.rand(B, T_) < 0.2) * 0.5
    h = rs.randint(1, hmax + 1, (B, T_)) + (rs.rand(B, T_) < 0.2) * 0.75
    if wide:
        w[rs.rand(B, T_) < wide] = W + 1
    return torch.as_tensor(np.stack((w, h), 1).astype(np.float32))


def run_unfolded(net, blocks, n):
    """PackRNN.forward's torch path -> dict of numpy arrays: cols (B, n), pos (B, T, 2), logp (B, n), reward (B,),
    margin (B, n) the top-two probability margin of every step, haps {type: (B, W')}"""
    margins = []
    hook = net.fc.register_forward_hook(lambda m, i, o: margins.append(np.diff(-o.detach().double().topk(2, dim=1).values.cpu().numpy(), axis=1)[:, 0]))
    try:
        with torch.no_grad():
            pos, logp, neg = net(blocks, n)
    finally:
        hook.remove()
    haps = {t: np.stack([net.engines[b].get_heightap(t) for b in range(len(net.engines))]) for t in ('full', 'zero', 'diff')}
    pos = pos.cpu().numpy()
    return {'cols': pos[:, :n, 0], 'pos': pos, 'logp': logp.cpu().numpy(), 'reward': -neg.cpu().numpy(),
            'margin': np.stack(margins, 1), 'haps': haps}


def compared(margin):
    """the margin rule -> keep (B, n) bool: the steps of every env that are compared; whole (B,) bool: envs not cut short"""
    low = margin < MARGIN
    first = np.where(low.any(axis=1), low.argmax(axis=1), margin.shape[1])
    keep = np.arange(margin.shape[1])[None, :] < first[:, None]
    return keep, first == margin.shape[1]


def assert_cap(whole):
    cut = int((~whole).sum())
    assert cut <= CAP * len(whole), "%d of %d envs cut short by the margin rule (cap %g)" % (cut, len(whole), CAP)
