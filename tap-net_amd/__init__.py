"""tap-net_amd -- MI355X-native batched Transport-and-Pack environment.

A drop-in for the packing hot path of Juzhan/TAP-Net (tools.Container, pack.update_dynamic /
update_mask / reward, PACKDataset) backed by hand-written HIP kernels behind the C ABI in
include/tapenv.h.  The directory name is not a Python identifier; import it as ``tap_net_amd``
(the alias module at the repository root) or via importlib.
"""
from . import _lib, build, datafiles, dist, env, generate, pack, rolling, rollout, synth, tools, trainer   # noqa: F401
from ._lib import TapError, TapOverflowError                   # noqa: F401
from .env import BatchedContainer, Container                   # noqa: F401
from .generate import generate_instances                       # noqa: F401
from .pack import (EnvTransition, EpisodeStepper, MaskStepper, PACKDataset, episode_scores, initial_mask, render, reward,   # noqa: F401
                   update_dynamic, update_mask)
from .rolling import RollingDataset, RollingStepper, RollingWindows, run_rolling_episode            # noqa: F401
from .rollout import (BestRatioPolicy, PointerHeadPolicy, RandomFeasiblePolicy, TapePolicy, UniformKeysPolicy,   # noqa: F401
                      UniformPickPolicy, critic_value, decoder_step, decoder_step_dropout, decoder_step_heightmap, decoder_step_heightmap_dropout,
                      dropout_keep_words, encode_dynamic_bits, pointer_pick, pointer_pick_draw, pointer_pick_given, pointer_pick_static, pointer_pick_static_supported, pointer_scores, pointer_scores_static, run_episode)
from .trainer import ClipAdam, TrainStep, reinforce_losses, reinforce_seeds, train, validate   # noqa: F401
from .tools import DRL, DynamicBitsEncoder, HeightmapEncoder, Pointer, RollingDRL, StateCritic, StaticFold, StepDropout, realCritic                # noqa: F401

__all__ = ["BatchedContainer", "Container", "MaskStepper", "EnvTransition", "EpisodeStepper", "PACKDataset", "initial_mask", "reward", "render", "episode_scores", "RollingDataset",
           "update_dynamic", "update_mask", "run_episode", "TapePolicy", "RandomFeasiblePolicy", "UniformPickPolicy", "UniformKeysPolicy",
           "BestRatioPolicy", "PointerHeadPolicy", "pointer_pick", "pointer_pick_draw", "pointer_pick_given", "pointer_pick_static", "pointer_pick_static_supported", "DRL", "RollingDRL", "encode_dynamic_bits", "DynamicBitsEncoder", "pointer_scores", "pointer_scores_static", "StaticFold", "decoder_step", "decoder_step_heightmap", "decoder_step_dropout", "decoder_step_heightmap_dropout", "dropout_keep_words", "StepDropout", "HeightmapEncoder", "Pointer", "critic_value", "StateCritic", "realCritic", "generate_instances", "RollingWindows", "RollingStepper", "run_rolling_episode", "TapError", "TapOverflowError",
           "ClipAdam", "TrainStep", "reinforce_losses", "reinforce_seeds", "train", "validate"]
