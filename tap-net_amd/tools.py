"""Names the reference's ``tools`` module exports on the hot path (model.py:4 does ``import tools``
and builds ``tools.Container`` per env, model.py:294), backed by the HIP kernels."""
import os

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from .env import BatchedContainer, Container, LockstepError, lockstep_containers, lockstep_scope   # noqa: F401
from .pack import reward as _reward            # noqa: F401


def calc_positions_lb_greedy(blocks, container_size, reward_type, device='cuda'):
    """tools.calc_positions_lb_greedy (tools.py:2393-2449) for one instance:
    -> positions (n, D) int, container=None (the voxel grid is never built), stable [n] bool,
    ratio = C+P+S (un-normalised), scores = [valid, box, empty, stable_num, max_h]."""
    blocks = np.asarray(blocks).astype('int')
    n, D = blocks.shape
    env = BatchedContainer(1, container_size, n, reward_type, 'full', device=device)
    for t in range(n):
        env.add_new_blocks(torch.as_tensor(blocks[t:t + 1].astype(np.int32)), want_feature=False)
    env.check()
    cnt = env.counters[0].tolist()
    hm = env.heightmap[0].cpu().numpy()
    max_h = int(hm.max())
    box = max_h * int(np.prod(container_size[:-1]))
    valid, empty, nst = cnt[0], cnt[1], cnt[2]
    ratio = (np.float64(valid) / np.float64(box) + np.float64(valid) / np.float64(empty + valid)) \
        + np.float64(nst) / np.float64(n)
    return (env.positions[0].cpu().numpy().astype(int), None, [bool(v) for v in env.stable[0].tolist()],
            float(ratio), [valid, box, empty, nst, max_h])


def is_stable_masks(bx, by, masks, use_lut=True, device='cuda'):
    """tools.is_stable (tools.py:710-765) for a batch of support patterns of one bx x by footprint that
    is off the floor: ``masks`` (n,) integers, bit (i*by + j) = footprint cell (i, j) rests on a voxel
    (tools.py:722-728).  -> (n,) bool tensor.  ``use_lut`` picks the table the 3D kernels use for
    footprints <= 4x4, False the direct form; both are the device functions the placements call."""
    dev = _lib.resolve_device(device)
    m = torch.as_tensor(np.asarray(masks, dtype=np.uint64).view(np.int64), device=dev).contiguous()
    out = torch.empty(m.numel(), dtype=torch.uint8, device=dev)
    c = _lib.ctx(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().tap_stable3d_eval(c, int(bx), int(by), _lib.ptr(m), m.numel(), 1 if use_lut else 0,
                                                _lib.ptr(out), _lib.stream_of(dev)), c)
    return out.bool()


class DQN(nn.Module):
    """The learned local pack-net ("L-Pnet", tools.DQN, tools.py:3322-3367): a column for a 2D block from the
    container's height-map.  Stock PyTorch; its parameter names and shapes are the reference's, so the SL / RL
    checkpoints load with ``load_state_dict(strict=True)``.  ``output_size`` = W columns; with ``is_diff_height`` the
    map's last entry (DRL_L's trailing 0 of the 'diff' form) is dropped.  forward(height_map (B, 1, W), block (B, 1, 2))
    -> (B, W) softmax probabilities."""

    def __init__(self, output_size, is_diff_height):
        super(DQN, self).__init__()
        self.conv_height_map = nn.Conv1d(1, 128, kernel_size=1)
        self.conv_block = nn.Conv1d(1, 128, kernel_size=1)
        self.bn1 = nn.BatchNorm1d(128)
        self.conv2 = nn.Conv1d(128, 256, kernel_size=1)
        self.bn2 = nn.BatchNorm1d(256)
        self.conv3 = nn.Conv1d(256, 256, kernel_size=1)
        self.bn3 = nn.BatchNorm1d(256)
        # positions along the conv axis: the map (W, or W - 1 with the diff input) and the block's two sides --
        # 1 536 / 1 792 inputs for the reference's W = 5
        self.lin1 = nn.Linear(256 * (output_size - (1 if is_diff_height else 0) + 2), 512)
        self.head = nn.Linear(512, output_size)
        self.is_diff_height = is_diff_height

    def forward(self, height_map, block):
        if self.is_diff_height:
            height_map = height_map[:, :, :-1]
        h = torch.cat((self.conv_height_map(height_map), self.conv_block(block)), dim=-1)
        h = F.relu(self.bn1(h))
        h = F.relu(self.bn2(self.conv2(h)))
        h = F.relu(self.bn3(self.conv3(h)))
        h = F.relu(self.lin1(h.reshape(h.size(0), -1)))
        return F.softmax(self.head(h), dim=1)


# the reference's checkpoint paths, relative to its working directory (tools.py:3544-3553)
PACK_NET_CHECKPOINTS = {'C+P+S-SL-soft': './pack_net/SL_rand_diff/checkpoints/199/SL.pt',
                        'C+P+S-RL-soft': './pack_net/RL_rand_diff/checkpoints/199/actor.pt'}


def load_pack_net(reward_type, container_width, device='cuda'):
    """DQN(W, True) in eval mode with the checkpoint tools.calc_positions_net loads for ``reward_type``."""
    if reward_type not in PACK_NET_CHECKPOINTS:
        raise NotImplementedError("the %s pack-net (calc_positions_LG_net) is outside this package" % reward_type)
    net = DQN(int(container_width), True)
    path = PACK_NET_CHECKPOINTS[reward_type]
    if not os.path.exists(path):
        raise FileNotFoundError("%s: the %s pack-net checkpoint (tools.py:3544-3553 loads it relative to the working "
                                "directory); pass net= instead" % (path, reward_type))
    net.load_state_dict(torch.load(path, map_location='cpu'))
    return net.to(_lib.resolve_device(device)).eval()


def calc_positions_net(blocks, container_size, reward_type, net=None, device='cuda'):
    """tools.calc_positions_net (tools.py:3506-3598) for one instance, SL / RL types: the pack-net picks every block's
    column from the raw height-map, the placement is tools.calc_one_position_net's (tapenv.h: TAP_AT_NET).
    -> positions (n, 2), container=None, stable [n] bool, ratio = (C+P+S)/3,
    scores = [valid, box, empty, stable_num, max_h].  ``net=None`` loads the reference's checkpoint."""
    from .pack import episode_scores_net
    if reward_type not in PACK_NET_CHECKPOINTS:
        raise NotImplementedError("the %s pack-net (calc_positions_LG_net) is outside this package" % reward_type)
    blocks = np.asarray(blocks).astype('int')
    n, D = blocks.shape
    if D != 2:
        raise NotImplementedError("calc_positions_net is 2D here (the reference's calc_one_position_net unpacks two sides)")
    dev = _lib.resolve_device(device)
    if net is None:
        net = load_pack_net(reward_type, container_size[0], dev)
    static = torch.zeros(1, 3, n, dtype=torch.float32)
    static[0, 1:, :] = torch.as_tensor(blocks.T.astype(np.float32))
    tour = torch.arange(n, dtype=torch.int64).unsqueeze(0)
    res = episode_scores_net(static.to(dev), tour.to(dev), reward_type, list(container_size), net, allow_rot=False,
                             with_env=True)
    ratio, scores, env = res
    return (env.positions[0].cpu().numpy().astype(int), None, [bool(v) for v in env.stable[0].tolist()],
            float(ratio[0].item()), [int(v) for v in scores[0].tolist()])
