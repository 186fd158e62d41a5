"""What tests/test_actor_reference_cpu.py and tests/test_actor_reference_gpu.py share: the fixtures that
tests/golden/make_golden_actor.py records from the reference's own actor (model.DRL.forward, model.py:254-515) and the
package modules that take its state dict between them."""
import os

import numpy as np
import torch
from torch import nn

import golden_util as G
import tap_net_amd as T
from tap_net_amd import tools

HE, HD, N = 32, 64, 10
BATCH = {2: 19, 3: 17}
CONTAINER = {2: [5, 50], 3: [5, 5, 50]}
CASES = [(2, "init"), (2, "sharp"), (3, "init"), (3, "sharp")]
N_KEYS = {2: 16, 3: 20}
SIZE_LIMIT = 770887                  # host_reference.npz, the largest fixture committed before these


def path(D, ws):
    return os.path.join(G.GOLDEN, "actor_%dd_%s.npz" % (D, ws))


_LOADED = {}


def load(D, ws):
    """the fixture's arrays as a dict, read once per process"""
    if (D, ws) not in _LOADED:
        with np.load(path(D, ws), allow_pickle=False) as z:
            _LOADED[(D, ws)] = {k: z[k] for k in z.files}
    return _LOADED[(D, ws)]


def instances(D):
    """the first B instances of the committed data set -> static (B, 1 + D, nR), dynamic (B, 3 n, nR) float32 numpy"""
    ds = G.load("dataset_%dd.npz" % D)
    B = BATCH[D]
    return ds["static"][:B].astype(np.float32), ds["dynamic"][:B].astype(np.float32)


def state_dict(z):
    return {k[len("sd_"):]: torch.from_numpy(z[k]) for k in z if k.startswith("sd_")}


def build(z, D):
    """-> ({state-dict prefix: package module}, the set of keys they took): every module loaded with strict=True from its
    part of the reference's state dict, float32, eval mode"""
    sd = state_dict(z)
    mods = {"static_encoder.conv.": nn.Conv1d(D, HE, 1),
            "dynamic_encoder.": T.DynamicBitsEncoder(3 * N, HE),
            "static_decoder.conv.": nn.Conv1d(D, HD // 2, 1),
            "pointer.": tools.Pointer(HE, HD, 'shape_heightmap', 'bot')}
    if D == 2:
        mods["dynamic_decoder.conv."] = nn.Conv1d(4, HD // 2, 1)
    else:
        mods["dynamic_decoder."] = tools.HeightmapEncoder(2, HD // 2, (5, 5))
    taken = set()
    for prefix, mod in mods.items():
        part = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        mod.load_state_dict(part, strict=True)           # no key of the module missing from the part, none of the part unexpected
        mod.eval()
        assert not taken & {prefix + k for k in part}
        taken |= {prefix + k for k in part}
    return mods, taken


def dynamic_decoder(mods):
    return mods["dynamic_decoder.conv."] if "dynamic_decoder.conv." in mods else mods["dynamic_decoder."]


def named_parameters(mods):
    """{the reference's state-dict key: the package's parameter}"""
    return {prefix + name: p for prefix, mod in mods.items() for name, p in mod.named_parameters()}


def ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))
