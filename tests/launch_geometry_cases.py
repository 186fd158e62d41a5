"""The shapes of tests/test_launch_geometry_gpu.py, and what each is there for: shared with tests/test_launch_geometry_cpu.py,
which asks the library (tapenv.h: tap_pointer_scores_geometry, tap_encode_bits_geometry -- host only, no GPU) for the launch
geometry of every one and fails when the list no longer reaches a class that the GPU tests are there to reach.

A pointer case is (B, nR, rows, Hd, S, (before, after)): S = 0 the ``proj`` form, S >= 1 the static-rows form; ``before``
the envs per workgroup that the batch asks for, ``after`` what the LDS budget leaves of them (before == after: no halving).
Every B is a multiple of 1024 plus 3 -- plus 2 where three envs per workgroup would divide that (3075 = 3 * 1025, 6147 =
3 * 2049) --, so the last workgroup is ragged wherever a workgroup takes more than one env."""

# the forward's shapes: 3, 4, 5 (more envs than wavefronts: the softmax loop's second round) and 8 envs per workgroup -- the
# benchmark's geometry, its 3D window, several columns per lane in the softmax (nR 68), two shadow planes with two hidden
# chunks --, and the halving loop's 10 -> 5 and 12 -> 6
_FW = [((3074, 20, 30, 128), (3, 3)), ((4099, 20, 30, 128), (4, 4)), ((5123, 4, 10, 64), (5, 5)), ((8195, 20, 30, 128), (8, 8)),
       ((8195, 60, 30, 128), (8, 8)), ((8195, 68, 63, 64), (8, 8)), ((8195, 4, 65, 128), (8, 8)), ((10243, 4, 64, 256), (10, 5)),
       ((12291, 4, 64, 128), (12, 6))]
# the backward's: no halving at 3, 8 and 5, then 3 -> 1, 4 -> 2, 6 -> 3, 8 -> 4
_BW = [((3074, 20, 30, 128), (3, 3)), ((8195, 20, 30, 128), (8, 8)), ((5123, 4, 10, 64), (5, 5)), ((3075, 32, 64, 256), (3, 1)),
       ((4099, 32, 64, 128), (4, 2)), ((6146, 20, 64, 128), (6, 3)), ((8195, 4, 64, 256), (8, 4))]

POINTER_FW = [s + (S, c) for S in (0, 2) for s, c in _FW] + \
    [(8195, 20, 30, 128, 5, (8, 8)), (9219, 4, 64, 256, 5, (9, 4))]       # S = 5: the LDS copy of G behind the per-env vectors
POINTER_BW = [s + (S, c) for S in (0, 2) for s, c in _BW] + [(2051, 100, 64, 256, 5, (2, 1))]

# the encoder, (B, nR, rows, H): forward at 3 (a full last workgroup, 3075, and a ragged one) and 8 envs per workgroup;
# backward at 9 envs per slice, and at 13 with three hidden chunks
ENCODER_FW = [(3075, 4, 10, 7), (3074, 4, 10, 7), (8195, 4, 10, 7)]
ENCODER_BW = [(8195, 4, 10, 7), (4099, 4, 128, 64)]

# the critic, (rows, nR, H, S, n, B): four envs per workgroup whatever the batch, so B = 131 gives 33 partials -- the second
# run of 32 of k_critic_value_bw_reduce -- and B = 4099 gives 1025
CRITIC_FW = [(10, 4, 64, 2, 1, 4099)]
CRITIC_BW = [(10, 4, 64, 2, 1, 131), (10, 4, 64, 2, 1, 4099)]

POINTER_NW = 4          # wavefronts per workgroup (pointer.hip: PTR_NW): more envs than this and the softmax loop goes round again
REDUCE_RUN = 32         # k_pointer_scores_bw_reduce and k_critic_value_bw_reduce add the partials in runs of 32


def case_id(c):
    return "-".join(str(v) for v in c[:5]) if len(c) == 6 and isinstance(c[5], tuple) else "-".join(str(v) for v in c)
