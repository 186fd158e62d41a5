#!/usr/bin/env python3
"""Generate tests/golden/rolling_actor_2d.npz by running the UPSTREAM REFERENCE's rolling actor, rolling.DRL
(rolling.py:201-460), in rolling.validate's loop (rolling.py:589-653) on the CPU: B = 5 instances of N = 20 blocks from the
reference's generator at a fixed seed (generate.generate_blocks, initial container 7 x 100, sizes 1 .. 5), windows of 10
(generate.InitialContainer), 2D, 'bot', rotations allowed, target container 5 x 100, 'diff', 'shape_heightmap', LB_GREEDY;
He = 32, Hd = 64 and the "sharp" scaling of make_golden_actor.py (one seeded xavier draw, then the two v times 300 and the
pointer's other matrices times 4).  The loop is restated here -- the reference's validate makes directories and draws --
statement by statement: convert_to_input, the forward with one_step until the last graph, a whole episode there, last_hh and
the decoder inputs carried, remove_block(sub_graph_nodes[ptr mod 10]); then the five figures of rolling.py:640-653.

Three runs per instance, as make_golden_actor.py does them and for its reason: float64 greedy (its picks are the recorded
tour), float64 with the pick forced to that tour (asserted equal to the greedy run bit for bit) and float32 forced -- the
stand-in for ``torch`` goes on rolling's namespace, where rolling.py:394 calls ``torch.max``.

Stored: the state dict (sd_<key>, float32); ctor_params, the names of rolling.DRL.__init__'s parameters in order; blocks and
positions (B, N, 2) as InitialContainer takes them; per step (B, N, ...) what the forward saw -- the window's ``static``, the
window tensor's bit shadow (pack.dynamic_bits layout, one word per column), ``current_mask``, ``decoder_static`` and
``decoder_dynamic`` -- and what it gave: ``logits``, ``last_hh``, the pick ``tour_idx`` and the global block id ``nodes``;
``tour_logp`` (float64); e_ref_logits / e_ref_last_hh per step (the float32 run against float64, the largest over the batch)
and e_ref_tour_logp; per instance valid_size, box_size, empty_size, stable_num, packing_height and the container's final
ratio.  Data only; members carry a fixed time stamp.  It runs only where the reference checkout is present.  Usage:

    python tests/golden/make_golden_rolling_actor.py
"""
import copy
import inspect
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
from make_golden_actor import HD, HE, SIZE_LIMIT, ForcedTorch, save, sharpen  # noqa: E402

B, N, CHILD, D = 5, 20, 10, 2
INIT, TARGET = [7, 100], [5, 100]
SEED = 6100
REWARD = "C+P+S-lb-soft"


def instances(generate):
    out = []
    for b in range(B):
        np.random.seed(SEED + b)
        rot_blocks, positions, _, _, _ = generate.generate_blocks(N, list(INIT), 1, [1, 5])
        blocks_all = np.asarray(rot_blocks).reshape(2, D, N).transpose(0, 2, 1).reshape(2 * N, D)      # rolling.py:484-486
        out.append((blocks_all, np.asarray(positions).reshape(D, N).T))                                # rolling.py:491-492
    return out


def shadow(dynamic):
    """(rows, nR) 0/1 -> (nR,) int64, bit r of word c = dynamic[r, c] (pack.dynamic_bits, rows <= 64)"""
    w = np.zeros(dynamic.shape[1], np.uint64)
    for r in range(dynamic.shape[0]):
        w |= (dynamic[r] != 0).astype(np.uint64) << np.uint64(r)
    return w.view(np.int64)


def initial_mask(torch, dynamic, n):
    move = dynamic[:, :n].sum(1); small = dynamic[:, n:2 * n].sum(1); large = dynamic[:, 2 * n:].sum(1)
    cur = torch.ones(dynamic.shape[0], dynamic.shape[2])
    cur[(small * large + move).ne(0)] = 0.                                                             # rolling.py:329-335
    return cur


def run(torch, rolling, tools, generate, pack, actor, dtype, inst, forced=None):
    """rolling.validate's loop for ONE instance on a copy of ``actor`` in ``dtype`` -> dict of per-step arrays and the figures"""
    net = copy.deepcopy(actor).to(dtype).eval()
    container = tools.Container(list(TARGET), N, REWARD, "diff", packing_strategy="LB_GREEDY")
    net.containers = [container]
    rec = dict(static=[], bits=[], current_mask=[], decoder_static=[], decoder_dynamic=[], logits=[], last_hh=[])
    state = {}

    def upd(dynamic_, static_, ptr, input_type, allow_rot):
        state["dynamic"] = pack.update_dynamic(dynamic_, static_, ptr, input_type, allow_rot)
        return state["dynamic"]

    def msk(mask_, dynamic_, static_, ptr, input_type, allow_rot):
        c, m = pack.update_mask(mask_, dynamic_, static_, ptr, input_type, allow_rot)
        state["current_mask"] = c
        return c, m

    net.update_fn, net.mask_fn = upd, msk

    def before_pointer(mod, ins):            # one call per decoding step: what this step sees
        rec["static"].append(state["static"].numpy()[0].astype(np.int16))
        rec["bits"].append(shadow(state["dynamic"].numpy()[0]))
        rec["current_mask"].append(state["current_mask"].numpy()[0].astype(np.uint8))

    def after_pointer(mod, ins, outs):
        rec["logits"].append(outs[0].detach().double().numpy()[0].copy())
        rec["last_hh"].append(outs[1].detach().double().numpy()[0, 0].copy())

    def before_static_decoder(mod, ins):
        rec["decoder_static"].append(ins[0].detach().numpy()[0].copy())
        return (ins[0].to(dtype),)

    def before_dynamic_decoder(mod, ins):
        rec["decoder_dynamic"].append(ins[0].detach().numpy()[0].copy())
        return (ins[0].to(dtype),)            # the reference hands it torch.FloatTensor(heightmaps) whatever the model's dtype is

    hooks = [net.pointer.register_forward_pre_hook(before_pointer), net.pointer.register_forward_hook(after_pointer),
             net.static_decoder.register_forward_pre_hook(before_static_decoder),
             net.dynamic_decoder.register_forward_pre_hook(before_dynamic_decoder)]
    ic = generate.InitialContainer(inst[0], inst[1], N, list(INIT), True, CHILD, "bot")
    real = rolling.torch
    stand_in = ForcedTorch(real, forced) if forced is not None else None
    picks, nodes = [], []
    try:
        if stand_in is not None:
            rolling.torch = stand_in
        with torch.no_grad():                                                                          # rolling.py:579-637
            one_step, last_hh = True, None
            decoder_static, decoder_dynamic = torch.zeros(1, D, 1), torch.zeros(1, TARGET[0] - 1, 1)
            while one_step:
                static, dynamic = ic.convert_to_input()
                static = torch.FloatTensor(static).unsqueeze(0).to(dtype)
                dynamic = torch.FloatTensor(dynamic).unsqueeze(0).to(dtype)
                if ic.is_last_graph():
                    one_step = False
                state.update(static=static, dynamic=dynamic, current_mask=initial_mask(torch, dynamic, CHILD))
                sub = list(ic.sub_graph_nodes)
                seen = len(rec["logits"])
                ptr, (decoder_static, decoder_dynamic), last_hh = net(static, dynamic, [decoder_static, decoder_dynamic], last_hh, one_step)
                steps = len(rec["logits"]) - seen
                assert steps == (1 if one_step else CHILD)
                if one_step:
                    p = int(ptr.numpy()[0])
                    picks.append(p)
                    nodes.append(sub[p % CHILD])
                    ic.remove_block(sub[p % CHILD])
                else:
                    state["last_sub"] = sub                               # (the forward returns only the last of these picks)
    finally:
        rolling.torch = real
        for h in hooks:
            h.remove()
    out = {k: np.stack(v) for k, v in rec.items()}
    assert out["logits"].shape == (N, 2 * CHILD)
    height = np.max(container.heightmap)
    out.update(picks=picks, nodes=nodes, last_sub=state["last_sub"],
               metrics=np.array([container.valid_size, TARGET[0] * height, container.empty_size,
                                 np.sum(container.stable) * (CHILD / N), container.bounding_box[-1]], np.float64),
               ratio=np.float64(container.calc_ratio()))
    return out


def greedy_picks(logits, current_mask):
    """torch.max(softmax(logits + log(mask)), 1)[1] of rolling.py:384-394 for recorded float64 steps: the first largest"""
    import torch
    probs = torch.softmax(torch.from_numpy(logits) + torch.from_numpy(current_mask.astype(np.float64)).log(), dim=1)
    return torch.max(probs, 1)[1].numpy()


def main():
    mods = ref_loader.load()
    if mods is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    tools, pack, generate = mods
    import torch
    torch.set_num_threads(1)
    sys.path.insert(0, ref_loader.REFERENCE_DIR)
    try:
        import rolling
    finally:
        sys.path.remove(ref_loader.REFERENCE_DIR)
    torch.manual_seed(SEED)
    actor = rolling.DRL(D, 3 * CHILD, HE, HD, False, "bot", True, TARGET[0], TARGET[1], D, REWARD, "shape_heightmap", "diff",
                        "LB_GREEDY", None, pack.update_dynamic, pack.update_mask, 1, 0.1, 1).eval()
    actor = sharpen(torch, actor, D)
    per = dict(f64=[], f32=[])
    for inst in instances(generate):
        greedy = run(torch, rolling, tools, generate, pack, actor, torch.float64, inst)
        # the whole tour of window-local picks: the one-step windows' returned picks, then the last graph's, which are the
        # greedy picks of its recorded steps
        last = greedy_picks(greedy["logits"][N - CHILD:], greedy["current_mask"][N - CHILD:])
        tour = np.concatenate((np.asarray(greedy["picks"], np.int64), last.astype(np.int64)))
        forced = torch.from_numpy(tour).unsqueeze(0)
        f64 = run(torch, rolling, tools, generate, pack, actor, torch.float64, inst, forced=forced)
        f32 = run(torch, rolling, tools, generate, pack, actor, torch.float32, inst, forced=forced)
        for k in ("static", "bits", "current_mask", "decoder_static", "decoder_dynamic", "logits", "last_hh", "metrics", "ratio"):
            assert np.array_equal(greedy[k], f64[k]), k                  # the forced float64 run IS the greedy one
        for k in ("static", "bits", "current_mask", "decoder_static", "decoder_dynamic", "metrics", "ratio"):
            assert np.array_equal(f32[k], f64[k]), k                     # ... and the float32 run saw the same windows
        assert f64["picks"] == list(tour[:N - CHILD])
        for r in (f64, f32):
            r["tour"] = tour
            r["nodes"] = np.asarray(list(r["nodes"]) + [r["last_sub"][p % CHILD] for p in tour[N - CHILD:]], np.int32)
            lg = torch.from_numpy(r["logits"]) + torch.from_numpy(r["current_mask"].astype(np.float64)).log()
            r["tour_logp"] = torch.log_softmax(lg, dim=1).gather(1, torch.from_numpy(tour).unsqueeze(1))[:, 0].numpy()
        assert sorted(f64["nodes"].tolist()) == list(range(N))
        per["f64"].append(f64)
        per["f32"].append(f32)
    st = lambda key, which="f64": np.stack([r[key] for r in per[which]])                                 # noqa: E731
    out = dict(ctor_params=np.asarray([p for p in inspect.signature(rolling.DRL.__init__).parameters if p != "self"]),
               blocks=np.stack([i[0][:N] for i in instances(generate)]).astype(np.int8),
               positions=np.stack([i[1] for i in instances(generate)]).astype(np.int16),
               initial_container_size=np.asarray(INIT), container_size=np.asarray(TARGET),
               static=st("static"), bits=st("bits"), current_mask=st("current_mask"),
               decoder_static=st("decoder_static").astype(np.int16), decoder_dynamic=st("decoder_dynamic").astype(np.int16),
               logits=st("logits"), last_hh=st("last_hh"), tour_idx=st("tour").astype(np.int16), nodes=st("nodes").astype(np.int16),
               tour_logp=st("tour_logp"), metrics=st("metrics"), ratio=st("ratio"),
               e_ref_logits=np.abs(st("logits", "f32") - st("logits")).max(axis=(0, 2)),
               e_ref_last_hh=np.abs(st("last_hh", "f32") - st("last_hh")).max(axis=(0, 2)),
               e_ref_tour_logp=np.abs(st("tour_logp", "f32") - st("tour_logp")).max())
    for name in ("decoder_static", "decoder_dynamic"):                   # integers: int16 holds them exactly
        assert np.array_equal(out[name].astype(np.float64), st(name).astype(np.float64)), name
    for k, v in actor.state_dict().items():
        out["sd_" + k] = v.numpy().astype(np.float32)
        assert np.array_equal(out["sd_" + k], v.numpy())
    peaks = np.abs(out["logits"]).max(axis=(0, 2))
    print("per-step max |logits| %.4g .. %.4g" % (peaks.min(), peaks.max()))
    print("e_ref: logits %.3g  last_hh %.3g  tour_logp %.3g" % (out["e_ref_logits"].max(), out["e_ref_last_hh"].max(), out["e_ref_tour_logp"]))
    print("metrics (valid, box, empty, stable, height):\n%s\nratio %s" % (out["metrics"], out["ratio"]))
    path = os.path.join(HERE, "rolling_actor_2d.npz")
    save(path, out)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    assert size < SIZE_LIMIT, size


if __name__ == "__main__":
    main()
