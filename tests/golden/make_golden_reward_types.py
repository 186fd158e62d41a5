#!/usr/bin/env python3
"""Generate tests/golden/reward_types.npz by running the UPSTREAM REFERENCE's tools.Container, tools.calc_positions_lb_greedy
and tools.calc_positions_mcs under the legacy reward names of tests/reward_type_cases.py ('comp', 'soft', 'hard', 'pyrm',
'pyrm-soft', 'pyrm-hard', 'pyrm-soft-sum', 'pyrm-hard-sum', 'pyrm-soft-SUM', 'pyrm-hard-SUM', 'CPS').  The blocks are
regenerated from seeds (reward_type_cases.Shape.blocks / golden_list) and not stored.

"traces" names one tools.Container run per (shape of GOLDEN_TRACES, name): all eleven names on the six lane-kernel
shapes, the five flag-class representatives on the wide ones, GOLDEN_B containers each, the feature type rotating through
diff / zero / full.  Rows trace_offsets[i] .. trace_offsets[i + 1] of "trace_digests" ((steps, 3, 6) uint8) hold, after
every add_new_block, 6-byte BLAKE2b digests of the int32 bytes of the GOLDEN_B containers' height-maps, of the feature
vectors add_new_block returned, and of positions[:t + 1] followed by stable[:t + 1]; the same rows of "trace_counters"
((steps, GOLDEN_B, 2) int16) hold valid_size and empty_size.  "trace_ratio" (traces, GOLDEN_B) and "trace_cps"
(traces, GOLDEN_B, 3) are calc_ratio() and calc_CPS() of the finished containers, float64.  Every block fits its container
and no container overflows: the script asserts that the reference raises nowhere in a trace.

One whole-episode call per entry of reward_type_cases.list_plan() (function, container, list, name; the names being the
eleven above and 'C+P-lb-soft'), in that order: "list_status" (uint8) is 0 where the reference returned, 1 where it raised
UnboundLocalError -- the function has no formula for the name (tools.py:2446 / :3311: every legacy name in
calc_positions_lb_greedy, 'C+P-lb-soft' in calc_positions_mcs) --, 2 where it raised IndexError -- the empty list
(tools.py:2417 / :3243 read blocks[0]).  For the calls that returned, in the same order, "list_ratio" (float64),
"list_scores" ((5,) int32: valid_size, box_size, empty_size, stable_num, height) and "list_digest" (8 bytes: positions
int32 then stable uint8) are what they returned.

A second run gives the same arrays (tests/test_reward_types_cpu.py checks that where the reference is present).  Usage:

    python tests/golden/make_golden_reward_types.py [output.npz]
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_loader  # noqa: E402
import reward_type_cases as RC  # noqa: E402


def main(path):
    mods = ref_loader.load()
    if mods is None:
        sys.exit("the reference checkout is not available (TAP_REFERENCE_DIR)")
    tools = mods[0]
    out, names, rows, counters, ratios, cpss = {}, [], [], [], [], []
    B = RC.GOLDEN_B
    for shape, name, feat in RC.trace_plan():
        blocks = shape.blocks(B)
        assert all((blocks[:, :, k] <= shape.cs[k]).all() for k in range(shape.D - 1)), "a block does not fit %s" % shape.name
        cons = [tools.Container(list(shape.cs), shape.n, name, feat, packing_strategy=shape.strategy) for _ in range(B)]
        steps, cnt = [], []
        for t in range(shape.n):
            with contextlib.redirect_stdout(io.StringIO()) as said:
                feats = [np.asarray(c.add_new_block(blocks[b, t].astype(np.float32), False)).reshape(-1) for b, c in enumerate(cons)]
            assert said.getvalue() == "", "the reference complains in %s / %s: %s" % (shape.name, name, said.getvalue()[:200])
            hm = np.stack([np.asarray(c.heightmap).reshape(-1) for c in cons])
            assert hm.max() <= shape.cs[-1], "%s overflows" % shape.name
            pos = np.stack([np.asarray(c.positions)[:t + 1] for c in cons])
            stb = np.stack([np.asarray(c.stable, dtype=bool)[:t + 1] for c in cons])
            steps.append(np.stack((RC.digest((hm, np.int32)), RC.digest((np.stack(feats), np.int32)),
                                   RC.digest((pos, np.int32), (stb, np.uint8))))[:, :RC.TRACE_DIGEST])
            cnt.append([[int(c.valid_size), int(c.empty_size)] for c in cons])
        rows.append(np.stack(steps))
        assert np.max(cnt) < 2 ** 15
        counters.append(np.asarray(cnt, np.int16))
        ratios.append([float(c.calc_ratio()) for c in cons])
        cpss.append([[float(v) for v in c.calc_CPS()] for c in cons])
        names.append(RC.trace_key(shape, name))
    out["traces"] = np.asarray(names).astype("S")
    out["trace_digests"] = np.concatenate(rows)
    out["trace_counters"] = np.concatenate(counters)
    out["trace_offsets"] = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    out["trace_ratio"] = np.asarray(ratios, np.float64)
    out["trace_cps"] = np.asarray(cpss, np.float64)

    status, lratio, lscores, ldigest = [], [], [], []
    for fn, cs, n, side, k, name in RC.list_plan():
        blocks = RC.golden_list(cs, n, side, k)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                positions, _, stable, ratio, sc = getattr(tools, fn)(blocks.astype(np.float32), list(cs), name)
        except (UnboundLocalError, IndexError) as e:
            status.append(RC.LIST_STATUS.index(type(e).__name__))
            continue
        status.append(0)
        lratio.append(float(ratio))
        lscores.append(np.asarray([int(v) for v in sc], np.int32))
        ldigest.append(RC.digest((positions, np.int32), (np.asarray(stable, dtype=bool), np.uint8)))
    out["list_status"] = np.asarray(status, np.uint8)
    out["list_ratio"] = np.asarray(lratio, np.float64)
    out["list_scores"] = np.stack(lscores)
    out["list_digest"] = np.stack(ldigest)
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "reward_types.npz"))
