#!/usr/bin/env python3
"""Generate tests/golden/window_forms.npz by running the UPSTREAM REFERENCE's pack.update_dynamic / pack.update_mask /
pack.reward on the window forms of tests/window_forms.py (R = 1, 'rot-old', 'bot'/False, the 3n-row input types,
'mul-with'), whose inputs are regenerated from seeds (window_forms.build) and not stored.

For every shape of window_forms.GOLDEN_CASES (B = 16, names in "cases"), along the case's tape, one row of 8-byte BLAKE2b
digests of the float32 bytes per recorded tensor (rows offsets[i] .. offsets[i + 1] of "digests", (1 + 3 * steps, 8) uint8):
    row 0               the mask DRL.forward starts from (model.py:297-307, restated below on the reference's tensors)
    rows 1 + 3t ..      after step t: pack.update_dynamic's output, then update_mask's new_mask (current_mask) and chosen_mask
The tensors themselves would make the fixture larger than every other mask fixture together; equal digests are equal bytes.

For the four tours of window_forms.TOURS on each container of TOUR_CONTAINERS (names in "tours"): "tour_reward"[k] =
pack.reward(...) as returned (float32, (B,)) and "tour_ratio"[k] = the float64 scores its calc_positions_* calls
returned ((B, 2): column 0, and for 'mul-with' one column per list, 0 for an empty one).  pack.reward names
tools.calc_positions_mus for the MACS strategy (pack.py:431), which the reference does not define; for the MACS tours this script binds that name to
tools.calc_positions_mcs while pack.reward runs -- the patch stays here.

The file is written without compression and with fixed zip timestamps, so a second run reproduces it byte for byte
(tests/test_window_forms_cpu.py checks that where the reference is present).  Usage:

    python tests/golden/make_golden_window_forms.py [output.npz]
"""
import hashlib
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402
import window_forms as WF  # noqa: E402


def digest(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a, dtype=np.float32).tobytes(), digest_size=8).digest(), np.uint8)


def write_npz(path, arrays):
    """np.savez without compression and with a fixed time stamp per member: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asarray(arrays[name]), allow_pickle=False)


def initial_mask(torch, dynamic, n):
    """The mask DRL.forward starts from (model.py:297-307), as tests/golden/make_golden.py states it -> (current_mask, mask)"""
    mask = torch.ones(dynamic.shape[0], dynamic.shape[2])
    move, small, large = (dynamic[:, s * n:(s + 1) * n].sum(1) for s in range(3))
    cur = mask.clone()
    cur[(small * large + move).ne(0)] = 0.
    return cur, mask


def main(path):
    mods = ref_loader.load()
    if mods is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    tools, pack = mods[0], mods[1]
    import torch
    out, names, digests = {}, [], []
    for c in WF.GOLDEN_CASES:
        inp = WF.build(c, seed=0)
        static, dynamic = torch.from_numpy(inp["static"].copy()), torch.from_numpy(inp["dynamic"].copy())
        tape = torch.from_numpy(inp["tape"].copy())
        cur, mask = initial_mask(torch, dynamic, c.n)
        rows = [digest(cur.numpy())]
        for t in range(c.nsteps):
            ptr = tape[:, t]
            dynamic = pack.update_dynamic(dynamic, static, ptr, c.input_type, c.allow_rot)
            cur, mask = pack.update_mask(mask, dynamic, static, ptr, c.input_type, c.allow_rot)
            rows += [digest(dynamic.numpy()), digest(cur.numpy()), digest(mask.numpy())]
        digests.append(np.stack(rows))
        names.append(c.name)
    out["cases"] = np.asarray(names).astype("S")
    out["digests"] = np.concatenate(digests)
    out["offsets"] = np.cumsum([0] + [len(d) for d in digests]).astype(np.int32)
    tours, rewards, ratios = [], [], []
    for form, strategy in WF.TOURS:
        for D, W in WF.TOUR_CONTAINERS:
            c = WF.tour_case(form, strategy, D, W)
            static, tour = WF.tour_inputs(c)
            seen = []
            fn_name = "calc_positions_mcs" if strategy == "MACS" else "calc_positions_lb_greedy"
            real = getattr(tools, fn_name)

            def logged(blocks, container_size, reward_type, _real=real, _seen=seen):
                res = _real(blocks, container_size, reward_type)
                _seen.append(float(res[3]))
                return res

            target = "calc_positions_mus" if strategy == "MACS" else fn_name       # pack.py:431 (sic)
            setattr(tools, target, logged)
            try:
                r = pack.reward(torch.from_numpy(static.copy()), torch.from_numpy(tour.copy()), c.reward, c.input_type,
                                c.allow_rot, W, WF.TOUR_H, packing_strategy=strategy)
            finally:
                if strategy == "MACS":
                    delattr(tools, target)
                else:
                    setattr(tools, fn_name, real)
            key = WF.tour_key(form, strategy, D, W)
            rewards.append(r.numpy().astype(np.float32))
            if form == "mul-with":
                # two calls per env, an empty list makes none (pack.py:461-468): rebuild the (B, 2) table from the ids
                ids = np.take_along_axis(static[:, -1, :], tour[:, :c.n], 1)
                ratio, k = np.zeros((c.B, 2), np.float64), 0
                for b in range(c.B):
                    for tgt in (0, 1):
                        if (ids[b] == tgt).any():
                            ratio[b, tgt] = seen[k]
                            k += 1
                assert k == len(seen)
            else:
                assert len(seen) == c.B
                ratio = np.stack((np.asarray(seen, np.float64), np.zeros(c.B)), 1)
            ratios.append(ratio)
            tours.append(key)
    out["tours"] = np.asarray(tours).astype("S")
    out["tour_reward"] = np.stack(rewards)
    out["tour_ratio"] = np.stack(ratios)
    write_npz(path, out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "window_forms.npz"))
