/*
 * tapenv.h -- C ABI of libtapenv.so: the MI355X (gfx950) batched Transport-and-Pack environment.
 *
 * This is the drop-in boundary for the reference's (Juzhan/TAP-Net) packing hot path.  The
 * reference has no FFI -- its seams are plain Python callables and one class -- so every entry
 * point below names the reference symbol (file:line) it replaces; INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - Plain C: pointers and sizes only, no torch / HIP types.  `stream` is a hipStream_t passed
 *     as void* (NULL = the null stream).  Every call is asynchronous on `stream` unless it says
 *     "synchronous".
 *   - All data pointers are DEVICE pointers; the caller owns every buffer (e.g. torch tensors).
 *     The library allocates nothing per call and keeps no reference to caller memory.
 *   - Return value: TAP_OK (0) or a negative TAP_E_* code; tap_last_error(ctx) gives a message.
 *   - A tap_ctx is bound to one device and is not thread-safe; distinct contexts are independent.
 *   - There is no CPU fallback: without a HIP device tap_ctx_create fails with TAP_E_NODEVICE.
 *
 * Per-env state is an opaque device blob of tap_env_state_bytes(desc) bytes holding only the
 * height-map, four counters, an error word and the placement history (layout: DESIGN.md).
 */
#ifndef TAPENV_H
#define TAPENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAP_ABI_VERSION 1

typedef struct tap_ctx tap_ctx;

enum {
    TAP_OK = 0,
    TAP_E_INVALID = -1,     /* bad argument */
    TAP_E_UNSUPPORTED = -2, /* valid in the reference, not implemented here (e.g. LB_GREEDY > 16384 cells) */
    TAP_E_HIP = -3,         /* HIP runtime error */
    TAP_E_OVERFLOW = -4,    /* a placement reached above H (reference: IndexError tools.py:2109 /
                               silent clipping tools.py:2169) */
    TAP_E_NODEVICE = -5,    /* no usable HIP device */
    TAP_E_STEPS = -6        /* add_new_block called more than blocks_num times (tools.py:3677) */
};

/* packing strategy, tools.py:3617-3620 / 3679-3690 */
enum { TAP_LB_GREEDY = 0, TAP_MACS = 1 /* 'MACS' and 'MUL' */,
       TAP_LB = 2 /* the legacy 'LB' (tools.py:1602-1955): voxel-level state, tap_env_step only */ };

/* flag word: the string tests the reference performs on reward_type */
enum {
    TAP_F_HARD = 1 << 0,     /* reward_type.endswith('hard')  tools.py:2113 */
    TAP_F_USE_P = 1 << 1,    /* 'P' in reward_type             tools.py:2135 */
    TAP_F_USE_S = 1 << 2,    /* 'S' in reward_type             tools.py:2138 */
    TAP_F_MCS_ZERO = 1 << 3, /* reward_type.startswith('mcs')  tools.py:2709 */
    TAP_F_MCS_TIE = 1 << 4,  /* 'mcs' in reward_type           tools.py:2718 */
    /* place-at semantics (tap_env_desc_set_place_at; never set by tap_env_desc_init) */
    TAP_F_AT_CONTAINER = 1 << 5,
    TAP_F_AT_NET = 1 << 6
};

/* semantics of tap_env_step_at*: the two seams of the learned local pack-net (reward types C+P+S-SL-soft /
 * C+P+S-RL-soft) that drop a block at a caller-chosen column */
enum { TAP_AT_CONTAINER = 1 /* tools.Container.add_new_block_at, tools.py:3746-3822 (DRL_L, model.py:1211) */,
       TAP_AT_NET = 2 /* tools.calc_one_position_net, tools.py:3371-3461 (calc_positions_net, pack.reward / render) */ };

/* Container.calc_ratio formula, tools.py:3907-3966 */
enum {
    TAP_R_C = 0, TAP_R_CxS, TAP_R_CP, TAP_R_CPxS, TAP_R_CPS, TAP_R_2CPS, TAP_R_CxPxS,
    TAP_R_CP_HALF /* 'C+P-lb-soft' -> (C+P)/2, every other mode divides by 3 */
};

/* heightmap_type, tools.py:3716-3744 */
enum { TAP_FEAT_FULL = 0, TAP_FEAT_ZERO = 1, TAP_FEAT_DIFF = 2 };

/* element type of the `blocks` argument */
enum { TAP_DT_F32 = 0, TAP_DT_I32 = 1 };

typedef struct tap_env_desc {
    int32_t B;          /* number of containers stepped in lock-step */
    int32_t D;          /* 2 | 3 */
    int32_t W, L, H;    /* container_size; L = 1 when D == 2 */
    int32_t n_max;      /* blocks_num */
    int32_t strategy;   /* TAP_LB_GREEDY | TAP_MACS | TAP_LB */
    int32_t flags;      /* TAP_F_* */
    int32_t ratio_mode; /* TAP_R_* */
    int32_t feature;    /* TAP_FEAT_* */
} tap_env_desc;

/* ---- library / context ---------------------------------------------------------------- */

int tap_abi_version(void);
const char *tap_status_string(int status);
/* synchronous.  device = HIP ordinal. */
int tap_ctx_create(int device, tap_ctx **out);
void tap_ctx_destroy(tap_ctx *ctx);
const char *tap_last_error(const tap_ctx *ctx);

/* Launch record of the precedence-update ("stream wave") kernels, for tests: every launch through the variant selector
 * (tap_stream_variant.h) counts one hit on the context under the key (kind, D, G, nc, mode, extra, wt) -- kind a
 * TapStreamKind, D / G the window dimension and lane group of the launcher's dispatch (0 where its table ignores them),
 * (nc, mode, extra) the instantiation, wt 1 for write-through stores, 0 for nontemporal ones.  A launch captured into a
 * hipGraph counts once, at capture.  tap_variant_hits writes up to `cap` rows of 8 ints (the key, then the count) and
 * returns the number of rows the record holds (TAP_E_INVALID if a key found no slot since the last reset);
 * tap_variant_hits_reset empties it. */
/* The whole-episode and rolling kernels count on the same record, under kinds 16 .. 33 (tap_common.h: TapHitKind; 25: trial.hip, 26: policy.hip, 27: encode.hip, 28: pointer.hip, 29: decoder.hip, 30: heightmap.hip, 31: critic.hip, 32: pack_rnn.hip, 33: dqn.hip), after
 * the stream-wave kinds 0 .. 6.  Their keys, fields (kind, D, G, nc, mode, extra, wt):
 *   16 k_episode<D, G, SOFT>                      (16, D, G, SOFT, 0, 0, 0)
 *   17 k_episode_macs2<G, WIDE>                   (17, 2, G, WIDE, 0, 0, 0)
 *   18 k_episode_macs3<G, WL>                     (18, 3, G, WL, 0, 0, 0)        WL = 5 for the 5 x 5 form, else 0
 *   19 k_rolling_step<D, G, CH> / _soft           (19, D, G, SOFT, CH, 0, wt)    SOFT 1 = k_rolling_step_soft; CH -2, 0, 10
 *   20 k_rolling_window<D, CH>                    (20, D, 0, 0, CH, 0, wt)       CH -2, 0, 10
 *      k_rolling_window_wide<D, NW>               (20, D, 0, 1, NW, 0, wt)       NW 3, 4
 *      k_rolling_window_big<D, MW>                (20, D, 0, 2, 0, MW, wt)       MW mask words 4, 16, 64
 *   21 k_rolling_init<D>                          (21, D, 0, 0, 0, 0, 0)
 *      k_rolling_init_big<D, MW>                  (21, D, 0, 1, 0, MW, 0)
 *   22 k_place_at<G, NET, ENG>                    (22, 2, G, SEM, GATHER, ENG, 0)  SEM a TAP_AT_*, GATHER 1 = _gather,
 *                                                 ENG 1 = tap_env_step_engine
 *   23 k_macs2d_wave_episode                      (23, 2, 64, 0, 0, PW, 0)       PW wavefronts (containers) per workgroup
 *   24 k_macs3d_wave_episode / _tight             (24, 3, 64, 0, TIGHT, PW, 0)   TIGHT 1 = the register-tight build (macs3_big.hip)
 *   25 k_trial_scores<D, G, HARD>                 (25, D, G, HARD, MASK, FRESH, 0) MASK 1 = a mask was given, FRESH 1 = TAP_T_FRESH
 *   26 k_policy_pick<G, GREEDY> / _wide<GREEDY>   (26, 0, G, GREEDY, PROBS, 0, 0) G 0 = the chunked form (nR > 64), PROBS 1 = probs_out given
 *      k_policy_pick_backward                     (26, 0, 0, 0, 0, 1, 0)
 *   27 k_encode_bits<HPL>                         (27, 0, HPL, PLANES, BIAS, 0, 0) HPL 1 | 2 hidden rows per lane, PLANES 1 | 2 shadow planes, BIAS 1 = a bias was given
 *      k_encode_bits_bw_partial + _reduce         (27, 0, 0, PLANES, BIAS, 1, 0) BIAS 1 = dbias wanted (one count per call)
 *   28 k_pointer_scores<HPL>                      (28, 0, HPL, PLANES, CHUNKS, 0, 0) CHUNKS = Hd / (64 HPL) hidden chunks per segment
 *      k_pointer_scores_bw<HPL> + _bw_reduce      (28, 0, HPL, PLANES, CHUNKS, 1, 0) (one count per call)
 *      k_pointer_scores<HPL, SS> / _bw<HPL, SS>   (28, 0, HPL, PLANES, CHUNKS, 0 | 1, S) the static-rows form, S = 1 .. 8 static rows (SS = S for 2, 3, 4, else 0)
 *   29 k_decoder_step                             (29, 0, TE, CHUNKS, H, 0, 0) TE = 16 envs per workgroup, CHUNKS = Hd / 64, H 1 = h given
 *      k_decoder_step_bw                          (29, 0, TE, CHUNKS, H, 1, 0)
 *   30 k_decoder_step_hm                          (30, C, NP, CHUNKS, H, 0, 0)   C height-map planes, NP = ceil(W / 4) ceil(L / 4) positions read
 *   31 k_critic_value<HPL>                        (31, RES, HPL, PLANES, MALL, 0, 0) HPL = H / 64 hidden rows per lane, RES 1 = U resident in LDS (0: recomputed per block), MALL 1 = all of M staged (0: a 64-row slab at a time)
 *      k_critic_value_bw<HPL> + _bw_reduce        (31, RES, HPL, PLANES, MALL, 1, 0) RES 1 = dU accumulated in LDS (0: in dU_out) (one count per call)
 *   32 k_pack_rnn_forward<KIND>                   (32, 2, TE, KIND, CHUNKS, 0, 0) TE = 16 envs per workgroup, KIND 0 = G, 1 = LG (TAP_PACK_*), CHUNKS = D / 64 = 4 | 6
 *   33 k_dqn_pick<TE>                             (33, 2, TE, DIFF, P, 0, 0)     TE = 16 | 8 envs per workgroup, DIFF 1 = the map's last entry is dropped, P = Wm + 2 positions
 * wt is the launch's RollArgs::wt (the window's fp32 stores; the init kernels store none), 0 for the episode kernels. */
int tap_variant_hits(tap_ctx *ctx, int32_t *out, int cap);
int tap_variant_hits_reset(tap_ctx *ctx);

/* ---- tools.Container, batched --------------------------------------------------------- */

/* Fill `d` from the arguments of tools.Container.__init__ (tools.py:3611-3661), performing its
 * string tests once on the host: container_size = D ints, reward_type e.g. "C+P+S-lb-soft",
 * heightmap_type "full"|"zero"|"diff", packing_strategy "LB_GREEDY"|"MACS"|"MUL"|"LB" (the reward
 * string overrides it exactly as tools.py:3617-3620 does).  Host only, no device work. */
int tap_env_desc_init(tap_env_desc *d, int B, int D, const int32_t *container_size, int blocks_num,
                      const char *reward_type, const char *heightmap_type,
                      const char *packing_strategy);

/* Place-at semantics for `d` (TAP_AT_CONTAINER | TAP_AT_NET, 0 = none): sets the TAP_F_AT_* bits of d->flags.  A
 * flagged descriptor is stepped by tap_env_step_at* only (tap_env_step* return TAP_E_INVALID for it) and its state
 * blob carries one more section, B x W int32 block cells per column, at its end.  2D only (TAP_E_INVALID for D = 3).
 * Host only. */
int tap_env_desc_set_place_at(tap_env_desc *d, int semantics);

/* bytes of device memory the caller must provide for the state blob (256-byte aligned) */
size_t tap_env_state_bytes(const tap_env_desc *d);
/* floats per env returned by step/feature: W*L (full/zero), W-1 (2D diff), 2*W*L (3D diff) */
int tap_env_feature_len(const tap_env_desc *d);

/* tools.Container.__init__ state / clear_container (tools.py:3629-3655, 3858-3885).  The blob is cleared by a
 * kernel, not hipMemsetAsync: the call may be captured into a hipGraph (a captured memset becomes a graph memset
 * node, which was observed to run out of order with the neighbouring kernel nodes on replay).  `state` must be
 * 16-byte aligned (TAP_E_INVALID otherwise). */
int tap_env_reset(tap_ctx *ctx, const tap_env_desc *d, void *state, void *stream);

/* tools.Container.add_new_block for all B envs (tools.py:3663-3744 -> calc_one_position_lb_greedy
 * 2027-2351, is_stable_2d 839-868, is_stable 710-765; with strategy TAP_MACS ->
 * calc_one_position_mcs_2d 2456-2749 / calc_one_position_mcs_3d 2751-3165 (2D: W <= 4096, H <= 4096 -- lane-per-column
 * kernels up to 16 columns, one wavefront per container above; 3D: W, L <= 64, H <= 4096 -- lane-per-cell kernel up to
 * 64 cells with sides <= 8, one wavefront per container above; block sides <= container sides, else error bit 4);
 * on the wave-per-container paths (LB_GREEDY and MACS 3D above 64 cells) tools.is_stable is evaluated for block
 * footprints up to 16 x 16 (csrc/tap_stable_wide.h beyond the 8 x 8 support masks), larger ones raise error bit 4;
 * LB_GREEDY containers up to 16384 cells (above 4096: one workgroup per container, the height-map in its LDS);
 * model.py:451-465 is the loop it replaces).
 *   blocks      (B, D) TAP_DT_F32 | TAP_DT_I32, one block per env; f32 is truncated like
 *               block.astype(int) (tools.py:3689)
 *   active      (B,) uint8 or NULL: envs with 0 are not stepped and only report their feature
 *               (the 'mul' input types' idle container, model.py:419-427)
 *   feature_out (B, feature_len) f32 or NULL: what add_new_block returns, already in the layout
 *               model.py:456-465 builds ((B,W-1,1) / (B,2,W,L) for 'diff') */
int tap_env_step(tap_ctx *ctx, const tap_env_desc *d, void *state, const void *blocks,
                 int blocks_dtype, const uint8_t *active, float *feature_out, void *stream);

/* Same, with the gather of model.py:404-412 fused in: block[k] = static_[b, 1+k, ptr[b]].
 * static_ (B, static_rows, nR) f32, ptr (B,) int64. */
int tap_env_step_gather(tap_ctx *ctx, const tap_env_desc *d, void *state, const float *static_,
                        int static_rows, int nR, const int64_t *ptr, const uint8_t *active,
                        float *feature_out, void *stream);

/* The pack-net placement (tools.Container.add_new_block_at, tools.py:3746-3822 / tools.calc_one_position_net,
 * tools.py:3371-3461, by the descriptor's TAP_F_AT_* semantics) for all B envs: block b goes to column pos_x[b]
 * (B,) int64, clamped to W - w like the reference's `while x + w > W: x -= 1`; z = max(heightmap[x:x+w]).
 * TAP_AT_CONTAINER: stable always (the reference tests the support row after filling it), empty_size += the filled
 * cells under the block counted again at every step (sum_c z - block cells of column c); TAP_AT_NET: stability of
 * the support row before the fill (tools.is_stable_2d), empty_size = sum(heightmap) - valid_size.  A column < 0 or a
 * block wider than W: error bit 4, not placed; z + h > H: error bit 1 (the reference clips silently), placed.
 * blocks / blocks_dtype / static_ / ptr / active / feature_out as tap_env_step / tap_env_step_gather.
 *   pnet_out   (B, 1, W) f32 or NULL: the pack-net's input for the NEXT step, from the state just written, in form
 *              pnet_form: TAP_FEAT_FULL (the raw height-map, tools.py:3407), TAP_FEAT_ZERO (minus its minimum) or
 *              TAP_FEAT_DIFF (hm[c+1] - hm[c] with a trailing 0, length W: DRL_L's transform, model.py:1188-1192)
 * TAP_E_INVALID for an unflagged descriptor or D = 3; TAP_E_UNSUPPORTED for W > 64.  One launch (lane per column). */
int tap_env_step_at(tap_ctx *ctx, const tap_env_desc *d, void *state, const void *blocks, int blocks_dtype,
                    const uint8_t *active, float *feature_out, const int64_t *pos_x, float *pnet_out, int pnet_form,
                    void *stream);
int tap_env_step_at_gather(tap_ctx *ctx, const tap_env_desc *d, void *state, const float *static_, int static_rows,
                           int nR, const int64_t *ptr, const uint8_t *active, float *feature_out, const int64_t *pos_x,
                           float *pnet_out, int pnet_form, void *stream);

/* The global pack-net's environment (pack_net/LG_RL.py: PackEngine.step, LG_RL.py:440-496; reward types C+P+S-G-soft
 * / C+P+S-LG-soft, the reference's DRL_RNN) at inner step `step` of a PackRNN forward, for all B envs of a TAP_AT_NET
 * descriptor whose tape holds at least T steps (n_max >= T).  Block b is blocks[b, :, step] of a (B, 2, T) f32 array,
 * truncated (block.int()); it goes to column pos_x[b] (B,) int64 with TAP_AT_NET's rules (clamp to W - w, z =
 * max(heightmap[x:x+w]), stability of the support row, empty_size = sum(heightmap) - valid_size).
 *   step % max_blocks == 0  the step starts from the empty container and reads nothing from the blob (the forward's
 *                           clear, LG_RL.py:610-614, and the engine's wrap); max_blocks = 0: never wraps, only step 0
 *   tape                    (x, z) and stability are recorded at index `step` ((0, 0), unstable, for a refused block);
 *                           the counters' 4th field is the forward's tape length, step + 1 (tap_env_export shows that
 *                           many rows); the error word restarts at step 0
 *   reward_out              (B,) f32 or NULL: (C + P + S) / 3 in fp64, stored as f32 -- C = valid / (max(hm) * W), P =
 *                           valid / (valid + empty), S = stable blocks / steps since the last clear (PackEngine counts
 *                           every step), C and P 0 when their denominator is 0 (LG_RL.py:460-475, 670)
 *   (step + 1) % max_blocks == 0  after the reward and the tape were taken, the engine clears (LG_RL.py:482-491): the
 *                           blob and feature_out hold the empty container
 *   feature_out             (B, W') f32 or NULL: the net's next input in the descriptor's heightmap_type form (the
 *                           layout tap_env_step writes; W' = W - 1 for diff)
 * A column < 0 or a block wider than W: error bit 4, not placed; z + h > H: error bit 1 (the reference clips its numpy
 * slices), placed.  TAP_E_INVALID for another descriptor, step outside [0, T) or beyond n_max, max_blocks < 0.  One
 * launch (k_place_at, lane per column). */
int tap_env_step_engine(tap_ctx *ctx, const tap_env_desc *d, void *state, const float *blocks, int T, int step,
                        int max_blocks, const int64_t *pos_x, float *feature_out, float *reward_out, void *stream);

/* tools.Container.get_heightmap (tools.py:3824-3856): the feature of the current state */
int tap_env_feature(tap_ctx *ctx, const tap_env_desc *d, const void *state, float *feature_out,
                    void *stream);

/* tools.Container.calc_ratio / calc_CPS (tools.py:3887-3966; model.py:499-510 stores it as fp32).
 * ratio_out (B,) f32, ratio64_out (B,) f64, cps_out (B,3) f64 -- each nullable. */
int tap_env_ratio(tap_ctx *ctx, const tap_env_desc *d, const void *state, float *ratio_out,
                  double *ratio64_out, double *cps_out, void *stream);

/* Container attributes in the reference's layouts (all nullable):
 * heightmap (B, W*L) i32; positions (B, n_max, D) i32; stable (B, n_max) u8;
 * counters (B, 4) i32 = valid_size, empty_size, sum(stable), current_blocks_num. */
int tap_env_export(tap_ctx *ctx, const tap_env_desc *d, const void *state, int32_t *heightmap_out,
                   int32_t *positions_out, uint8_t *stable_out, int32_t *counters_out,
                   void *stream);

/* tools.is_stable (tools.py:710-765) evaluated mask by mask, for tests of the predicate itself: the
 * placement kernels call the same two device functions.  masks (n,) uint64, bit (i*by + j) = footprint
 * cell (i, j) of a bx x by block rests on a voxel (tools.py:722-728); the block is off the floor.
 * use_lut != 0: through the per-context table the 3D kernels use for footprints <= 4x4 (larger ones
 * fall through to the direct form, as in the kernels); 0: the direct hull-free form only.
 * stable_out (n,) uint8.  bx, by <= 8. */
int tap_stable3d_eval(tap_ctx *ctx, int bx, int by, const unsigned long long *masks, int n,
                      int use_lut, uint8_t *stable_out, void *stream);

/* The containers' sticky error words, asynchronously: err_out (B,) int32 with bit 1 = a placement reached above H
 * (the reference raises IndexError, tools.py:2109), 2 = add_new_block called more than blocks_num times, 4 = bad
 * block / column index, 8 / 16 = MACS list guards.  For callers that report per container instead of raising. */
int tap_env_errors(tap_ctx *ctx, const tap_env_desc *d, const void *state, int32_t *err_out, void *stream);

/* Synchronous.  Returns TAP_OK, or TAP_E_OVERFLOW / TAP_E_STEPS if any env has raised its sticky
 * error word; *n_bad_out (host, nullable) = number of such envs. */
int tap_env_check(tap_ctx *ctx, const tap_env_desc *d, const void *state, int32_t *n_bad_out,
                  void *stream);

/* pack.reward (pack.py:378-473) == tools.calc_positions_lb_greedy (tools.py:2393-2449) per env:
 * the whole episode in one launch.  static_ (B, static_rows, nR) f32, tour (B, n) int64,
 * reward_out (B,) f32 = -(C+P+S) un-normalised; positions_out (B, n, D) i32 and stable_out
 * (B, n) u8 nullable.  d->B is ignored (B given here); no state blob is needed.  LB_GREEDY only (pack.py:431 names a
 * function the reference does not have for MACS / MUL: TAP_E_UNSUPPORTED; tap_episode_scores packs with them). */
int tap_episode_reward(tap_ctx *ctx, const tap_env_desc *d, int B, int n, const float *static_,
                       int static_rows, int nR, const int64_t *tour, float *reward_out,
                       int32_t *positions_out, uint8_t *stable_out, void *stream);

/* tools.calc_positions_lb_greedy (tools.py:2393-2449) / tools.calc_positions_mcs (tools.py:3213-3315) per env,
 * as pack.render calls them for its metric files (pack.py:743-792; caller trainer.py:132, 493): the whole
 * episode in one launch with every strategy tap_env_step has except the legacy 'LB' (render never uses it,
 * pack.py:741), containers of every size the step entry points take: lane-per-cell groups up to 64 cells, above that
 * (2D: above 64 columns; 3D: above 64 cells or a side above 8) one wavefront per container with its tile in LDS across
 * the n placements (LB_GREEDY: big.hip; MACS / MUL: macs_big.hip k_macs2d_wave_episode, macs3_big.hip
 * k_macs3d_wave_episode).  TAP_E_UNSUPPORTED only where that tile does not fit a workgroup's LDS or under
 * TAP_NO_WAVE_KERNELS: step those with tap_env_step_gather.  static_ / tour as tap_episode_reward.
 *   target_sel   -1: every tour entry.  0 | 1: the two-container input types ('mul', 'mul-with', pack.py:755-790):
 *                only the entries whose target id -- the LAST row of static_ -- equals it, in tour order.
 *   ratio64_out  (B,) f64: the function's `ratio` (tools.py:2442-2445 C+P+S; tools.py:3279-3308 by reward type,
 *                d->ratio_mode without Container.calc_ratio's division); 0 for an empty list (pack.py:760-769);
 *                NaN when the container raised an error bit
 *   scores_out   (B, 5) int64: valid_size, box_size, empty_size, stable_num, max(heightmap) (tools.py:2447, 3311);
 *                zeros for an empty list
 *   err_out      (B,) int32: the sticky error bits tap_env_check reports (1 overflow, 4 bad block / index, 8 / 16 MACS)
 * every output is nullable; positions_out (B, n, D) / stable_out (B, n) are indexed by tour position (entries of
 * the other container stay 0). */
int tap_episode_scores(tap_ctx *ctx, const tap_env_desc *d, int B, int n, const float *static_,
                       int static_rows, int nR, const int64_t *tour, int target_sel, double *ratio64_out,
                       int64_t *scores_out, int32_t *positions_out, uint8_t *stable_out, int32_t *err_out,
                       void *stream);

/* ---- instance generation (generate.py:773-971) ---------------------------------------- */

/* tools.calc_positions_lb_greedy (tools.py:2393-2449) for B explicit block lists: blocks (B, n, D)
 * int32 in placement order, one launch.  This is what generate.generate_blocks calls with
 * 'C+P+S-lb-hard' on the initial container (generate.py:908); an instance is accepted when every
 * stable_out flag is 1 (generate.py:909-910).  With strategy TAP_MACS: tools.calc_positions_mcs
 * (tools.py:3213-3315).  LB_GREEDY containers of any size (generate.py:908 accepts any --initial_container_width):
 * lane-per-cell groups up to 64 cells, above that one wavefront per container with the height-map in LDS across the n
 * placements (big.hip: k_big_wave_episode; above 4096 cells one workgroup per container, k_big_wg_episode, up to
 * 16384; tap_episode_reward / tap_episode_scores take the same path); MACS / MUL above 64 cells (2D: 64 columns; or a
 * 3D side above 8) likewise one wavefront per container, its height-map, history and lists in LDS across the n
 * placements (k_macs2d_wave_episode / k_macs3d_wave_episode; TAP_E_UNSUPPORTED only when that tile does not fit a
 * workgroup's LDS or under TAP_NO_WAVE_KERNELS: step those with tap_env_step_gather).  reward_out (B,) f32 = -score,
 * positions_out (B, n, D) i32, stable_out (B, n) u8, score64_out (B,) f64 = C+P+S (MACS / MUL: the function's `ratio` by
 * reward type, NaN where the container raised an error bit) -- each nullable.
 * A block with a side < 1 is not part of its list (lists of different length in one batch: the
 * two-container reward of pack.py:451-466 packs the blocks of each target id separately); S is
 * taken over the blocks that are, and an empty list scores 0 (pack.py:459-460). */
int tap_pack_blocks(tap_ctx *ctx, const tap_env_desc *d, int B, int n, const int32_t *blocks,
                    float *reward_out, int32_t *positions_out, uint8_t *stable_out,
                    double *score64_out, void *stream);

/* generate.calc_dependent (generate.py:575-771) + the rotation bookkeeping of
 * generate.generate_blocks (generate.py:935-971) + pack.PACKDataset's layout (pack.py:101-195,
 * input_type 'bot', allow_rot=True): from blocks and positions (B, n, D) i32 of fully packed
 * initial containers to static_out (B, 1+D, n*R) and dynamic_out (B, 3n, n*R) f32.
 * container_size = D host ints (the INITIAL container); arm_size as generate.py:623-641 (2D).
 * n <= 64. */
int tap_precedence(tap_ctx *ctx, int B, int D, int n, const int32_t *container_size, int arm_size,
                   const int32_t *blocks, const int32_t *positions, float *static_out,
                   float *dynamic_out, void *stream);

/* ---- perfect-packing ("PPSG") instances (generate.py:17-301) -------------------------------- */
/* Random draws are made the way numpy's RandomState makes them (random_sample, masked-rejection randint,
 * choice(p) by searchsorted on the fp64 cumulative sum) on counter-based word streams: word i of the stream
 * with key k = high 32 bits of splitmix64-finalise(k + i * 0x9E3779B97F4A7C15), k = key(seed, a, b, c) as
 * csrc/ppsg.hip / oracle/tap_oracle.c define it.  ids (B,) int64 = global instance ids (nullable:
 * instance0 + b), so any sharding generates the same instances. */

/* generate.BPP_Generator_3D (generate.py:232-301) inside generate_blocks_with_GT's acceptance loop
 * (generate.py:66-73): for every instance S slabs of ns <= 16 blocks, slab s = n - 1 guillotine cuts of a
 * W x W x heights[b, s] box, re-drawn (attempt a = 0, 1, ...; stream key(seed, id*S + s, gen, a)) until every
 * side is in [min_size, max_size); the slabs are stacked along z -- S = 1 is the reference's generator,
 * S > 1 builds perfect packings of S*ns blocks, which the reference's single rejection loop cannot reach
 * (acceptance < 2e-8 at 50 blocks).  gt_blocks_out / gt_positions_out (B, S*ns, 3) i32; attempts_out (B, S)
 * i32 nullable (-1 = max_attempts reached, that slab is then invalid). */
int tap_ppsg_gt(tap_ctx *ctx, int B, int S, int ns, int W, const int32_t *heights, int min_size,
                int max_size, uint64_t seed, const int64_t *ids, int64_t instance0, int gen,
                int64_t max_attempts, int32_t *gt_blocks_out, int32_t *gt_positions_out,
                int32_t *attempts_out, void *stream);

/* generate.py:86-105: a random order in which the perfect packing can be taken apart from the top and a
 * random rotation per block (stream key(seed, id, gen, 1000 + trial)) -> blocks_out (B, n, 3) i32 in layout
 * order, to be packed into the initial container with tap_pack_blocks ('C+P+S-lb-hard').  n <= 64. */
int tap_ppsg_order(tap_ctx *ctx, int B, int n, const int32_t *gt_blocks, const int32_t *gt_positions,
                   uint64_t seed, const int64_t *ids, int64_t instance0, int gen, int trial,
                   int32_t *blocks_out, void *stream);

/* The 2D forms (generate_blocks_with_GT with block_dim 2, generate.py:72-73): tap_ppsg_gt2d = generate.
 * BPP_Generator_2D_easy (generate.py:392-484) for B instances -- n - 1 guillotine cuts of a W x heights[b] box
 * (volume-weighted choice among the blocks with a side >= max_size, else among the splittable ones; the axis
 * rule of :446-454; uniform split positions for short sides, Gaussian ones from `gauss` for sides
 * >= 2*max_size - 1), re-drawn (stream key(seed, id, gen, attempt)) until every side is in [min_size, max_size).
 * gauss (gauss_rows, gauss_stride) f64, device: row L = the normalised cumulative sum np.random.choice makes
 * of the reference's Gaussian weights over the L - 2*min_size split positions of a side of length L (the
 * caller builds it with numpy, tap-net_amd/generate.py gauss_split_table; rows below 2*max_size - 1 unused).
 * gt_blocks_out / gt_positions_out (B, n, 2) i32; attempts_out (B,) i32 nullable, -1 = cap reached.
 * tap_ppsg_order2d = tap_ppsg_order on (B, n, 2) arrays with calc_dependent's 2D movement rule
 * (generate.py:575-647) and the two 2D rotations.  The layout test is tap_ppsg_check on the relations of the
 * 2D layout (forward / backward masks are empty there). */
int tap_ppsg_gt2d(tap_ctx *ctx, int B, int n, int W, const int32_t *heights, int min_size, int max_size,
                  const double *gauss, int gauss_stride, int gauss_rows, uint64_t seed, const int64_t *ids,
                  int64_t instance0, int gen, int64_t max_attempts, int32_t *gt_blocks_out,
                  int32_t *gt_positions_out, int32_t *attempts_out, void *stream);
int tap_ppsg_order2d(tap_ctx *ctx, int B, int n, const int32_t *gt_blocks, const int32_t *gt_positions,
                     uint64_t seed, const int64_t *ids, int64_t instance0, int gen, int trial,
                     int32_t *blocks_out, void *stream);

/* generate.py:110-156: accept a packed layout iff every block is stable (stable (B, n) u8 of
 * tap_pack_blocks) and the blocks can be taken out again last-packed-first (rel (B, 5, n) u64 of
 * tap_rolling_init: nothing on top, one free side per horizontal axis; input_simple != 0 ignores the
 * sides).  ok_out (B,) u8. */
int tap_ppsg_check(tap_ctx *ctx, int B, int n, int input_simple, const uint64_t *rel, const uint8_t *stable,
                   uint8_t *ok_out, void *stream);

/* ---- rolling precedence windows (generate.py:1589-1839, rolling.py:589-637) ------------- */

/* generate.InitialContainer.__init__: the five dependency graphs of B fully packed initial
 * containers with N <= 4096 blocks each, as column masks of NW = ceil(N/64) uint64 words with bit a of a
 * node j's mask = "block a blocks block j": rel_out holds 5*N*NW words per instance -- first the N movement
 * masks, then one record of four masks (left, right, forward, backward) per node, so that a step reads the
 * window nodes' side masks as one piece of a cache line each; state_out holds 2*NW words (entered, window).
 * Up to 64 blocks an instance is handled by one wavefront (lane = node), up to 256 blocks with windows of at
 * most 64 / NW nodes still by one wavefront (lane = NW nodes, NW-word masks; tap_rolling_step is one launch up to
 * 128 blocks and two above); wider windows and instances of 257 .. 4096 blocks by one thread per instance
 * (rolling.py:831 leaves --total_blocks_num free).  state_out is cleared. */
int tap_rolling_init(tap_ctx *ctx, int B, int D, int N, const int32_t *container_size, int arm_size,
                     const int32_t *blocks, const int32_t *positions, uint64_t *rel_out,
                     uint64_t *state_out, void *stream);

/* One step of rolling.validate's loop: InitialContainer.remove_block for the column picked in the
 * previous window (remove_ptr (B,) int64, NULL on the first call), then convert_to_input():
 * top the window up to `child` nodes and emit static_out (B, 1+D, child*R), dynamic_out
 * (B, 3*child, child*R) f32.  Optional by-products: colsum_out (B, 3, child*R) (the column sums
 * update_mask needs), bits_out (B, child*R) uint64 (the bit shadow of dynamic_out for
 * tap_transition_bits / tap_mask_step_bits; needs 3*child <= 64, child*R % 4 == 0), current_mask_out (B, child*R) (model.py:297-307), nodes_out (B, child) i32
 * (sorted global block ids = static's columns), err_out (B,) i32 (1 = window could not be filled).
 * dynamic_out may be NULL when bits_out is given: the window's precedence tensor then only exists as its bit shadow
 * (no fp32 expansion -- 7 200 of the 9 937 bytes a c5 step moves; for policies that read the shadow, as
 * tap_stepper_buffers.dyn = NULL for the decoding step).  tap_rolling_step and tap_roller_buffers.dynamic alike. */
int tap_rolling_window(tap_ctx *ctx, int B, int D, int N, int child, const int32_t *blocks,
                       const uint64_t *rel, uint64_t *state, const int64_t *remove_ptr,
                       float *static_out, float *dynamic_out, float *colsum_out, uint64_t *bits_out,
                       float *current_mask_out, int32_t *nodes_out, int32_t *err_out, void *stream);

/* One decoding step of rolling.validate in one launch: add_new_block for the column `ptr` picked
 * in the CURRENT window (block gathered from static_cur, the tensor tap_rolling_window / _step
 * wrote last) fused with remove_block + convert_to_input() for the NEXT window (written to
 * static_next, which must be a different buffer).  feature_out as in tap_env_step.  One kernel for LB_GREEDY on
 * containers of at most 64 cells and instances of at most 128 blocks (windows of at most 32 nodes above 64 blocks);
 * otherwise the two launches behind this entry. */
int tap_rolling_step(tap_ctx *ctx, const tap_env_desc *d, void *env_state, int N, int child,
                     const int32_t *blocks, const uint64_t *rel, uint64_t *state, const int64_t *ptr,
                     const float *static_cur, float *static_next, float *dynamic_out,
                     float *colsum_out, uint64_t *bits_out, float *current_mask_out, int32_t *nodes_out,
                     int32_t *err_out, float *feature_out, void *stream);

/* ---- precedence tensors (pack.py:276-376, model.py:297-307) --------------------------- */
/* dynamic is (B, rows, nR) f32 with rows = 3n ('bot', 'mul') or n ('simple', 'rot'); nR = n*R.
 * colsum is a (B, 3, nR) f32 shadow of the three per-section column sums of a dynamic tensor
 * (move / small / large, pack.py:324-326); sections beyond `rows` sum to 0. */

/* colsum_out = column sums of dynamic */
int tap_dyn_colsum(tap_ctx *ctx, int B, int n, int nR, int rows, const float *dynamic,
                   float *colsum_out, void *stream);

/* pack.update_dynamic (pack.py:333-376): dyn_out = dyn_in with rows real + n*i (i < update_rows)
 * zeroed, real = (long)static_[b, 0, ptr[b]].  Out of place.  If colsum_in/out are given the
 * shadow is updated incrementally (no reduction). */
int tap_update_dynamic(tap_ctx *ctx, int B, int n, int nR, int rows, int update_rows,
                       const float *dyn_in, const float *static_, int static_rows,
                       const int64_t *ptr, float *dyn_out, const float *colsum_in,
                       float *colsum_out, void *stream);

/* pack.update_mask (pack.py:276-331) from the column sums of the (already updated) dynamic.
 * ptr == NULL gives the initial mask of model.py:297-307 (mask_in may then be NULL = ones).
 * current_out = new_mask.float(), mask_out = chosen_mask. */
int tap_update_mask(tap_ctx *ctx, int B, int n, int R, const float *mask_in, const float *colsum,
                    const int64_t *ptr, float *current_out, float *mask_out, void *stream);

/* update_dynamic + update_mask in one launch (what model.py:376-386 does per step). */
int tap_mask_step(tap_ctx *ctx, int B, int n, int R, int rows, int update_rows,
                  const float *dyn_in, const float *static_, int static_rows, const int64_t *ptr,
                  const float *mask_in, const float *colsum_in, float *dyn_out, float *colsum_out,
                  float *current_out, float *mask_out, void *stream);

/* ---- the same two seams on a bit shadow of `dynamic` ------------------------------------ */
/* `dynamic` only ever holds 0 and 1 (the precedence matrices PACKDataset builds, pack.py:101-195;
 * update_dynamic only writes zeros, pack.py:370-374).  Carried as a (B, nR) uint64 shadow -- word j
 * of env b = column j, bit r = dynamic[b, r, j] != 0; for 65 <= rows <= 128 (windows of 22 .. 42 nodes) the
 * shadow is (B, 2, nR): plane 0 = rows 0..63, plane 1 = rows 64..127 -- a step no longer re-reads the
 * fp32 tensor: clearing the chosen rows is an AND, the column sums of pack.py:323-326 are popcounts,
 * and the fp32 tensor the network consumes next (model.py:378) is expanded from the bits, so the
 * step WRITES rows*nR*4 bytes per env and reads nR*8.  Outputs are bit-identical to tap_mask_step /
 * tap_transition for 0/1 input. */

/* uint64 words PER ENV of the shadow of a (rows, nR) window: nR up to 64 rows, 2 * nR for 65 .. 128 rows, 0 when the
 * shape has no shadow.  Every bits_in / bits_out buffer below holds B * tap_bits_words(rows, nR) words; the library
 * cannot see the allocation, so size it with this. */
int tap_bits_words(int rows, int nR);

/* bits_out (B, tap_bits_words(rows, nR)) = shadow of dynamic; *nonbinary_out (device int32, nullable, caller zeroes
 * it) is incremented by the number of elements that are neither 0 nor 1 -- the shadow is only valid at 0.
 * bits_out NULL: count only (then rows may exceed 128). */
int tap_dyn_bits(tap_ctx *ctx, int B, int nR, int rows, const float *dynamic,
                 unsigned long long *bits_out, int32_t *nonbinary_out, void *stream);

/* tap_mask_step on the shadow (bits_in / bits_out: B * tap_bits_words(rows, nR) words each).  Every output is nullable (at least one must be given) and mask_in
 * NULL means ones, so the same entry serves pack.update_dynamic alone (no mask outputs) and
 * pack.update_mask alone (update_rows = 0, masks only); ptr NULL (with update_rows = 0; static_ is then
 * unused) gives the initial mask of model.py:297-307.  A ptr outside [0, nR) -- the reference's gather
 * raises -- clears no row and removes no column, here and in tap_update_dynamic / tap_mask_step /
 * tap_transition* (whose placement half also raises error bit 4 for it).  Requires nR % 4 == 0, nR <= 256,
 * rows <= 128, 16-byte aligned buffers, bits_in != bits_out. */
int tap_mask_step_bits(tap_ctx *ctx, int B, int n, int R, int rows, int update_rows,
                       const unsigned long long *bits_in, const float *static_, int static_rows,
                       const int64_t *ptr, const float *mask_in, unsigned long long *bits_out,
                       float *dyn_out, float *current_out, float *mask_out, void *stream);

/* The FIRST step of an episode on a fresh fp32 `dynamic` (what PACKDataset / a DataLoader hands over,
 * pack.py:195): tap_mask_step_bits with the shadow built from dyn_in inside the launch (one read of the
 * tensor), so an episode needs no separate tap_dyn_bits pass.  bits_out receives the shadow of dyn_out;
 * *nonbinary_out (device int32, nullable, caller zeroes it) counts the elements of dyn_in that are neither
 * 0 nor 1 -- every output of the launch is only valid when it stays 0.  ptr NULL (update_rows = 0):
 * shadow + initial mask only. */
int tap_mask_step_first(tap_ctx *ctx, int B, int n, int R, int rows, int update_rows, const float *dyn_in,
                        const float *static_, int static_rows, const int64_t *ptr, const float *mask_in,
                        unsigned long long *bits_out, float *dyn_out, float *current_out, float *mask_out,
                        int32_t *nonbinary_out, void *stream);

/* ---- one whole lock-step in one launch --------------------------------------------------- */

enum {
    TAP_T_FRESH = 1, /* treat the state blob as freshly reset (Container.__init__, model.py:294) */
    TAP_T_RATIO = 2  /* also emit Container.calc_ratio after the step (model.py:499-510) */
};

/* Everything DRL.forward does around its policy network for one decoding step (model.py:376-465):
 * tap_mask_step + tap_env_step_gather fused, so the placement's latency hides under the HBM-bound
 * precedence update and a kernel boundary disappears.  n = blocks in the precedence window
 * (nR = n*R columns); d->n_max may be larger (rolling windows over one long-lived container).
 * One kernel for LB_GREEDY (2D/3D, up to 64 cells) and MACS/MUL (2D up to 16 columns; 3D up to 8 x 8), as long as a workgroup's candidate lists fit the device's LDS (160 KiB per workgroup on gfx950); every other
 * shape and strategy tap_env_step takes (legacy 'LB', LB_GREEDY and MACS 3D above 64 cells, MACS 2D above 16 columns, a MACS
 * container whose candidate lists do not fit a fused workgroup's LDS) runs the same step as its two launches behind
 * this entry -- except on the bit shadow (tap_transition_bits / _first, the stepper), where the wave-per-container
 * shapes are one launch too since round 5: a container's wavefront runs its own precedence slab, then its placement
 * (big.hip, macs_big.hip, macs3_big.hip; for MACS a fresh container and calc_ratio stay launches of their own at the
 * two ends of an episode).  feature_out nullable; ratio_out (B,) f32 required with
 * TAP_T_RATIO. */
int tap_transition(tap_ctx *ctx, const tap_env_desc *d, void *state, int n, int R, int rows,
                   int update_rows, const float *dyn_in, const float *static_, int static_rows,
                   const int64_t *ptr, const float *mask_in, const float *colsum_in,
                   float *dyn_out, float *colsum_out, float *current_out, float *mask_out,
                   float *feature_out, float *ratio_out, int flags, void *stream);

/* 1 when the tap_transition* entry points run a step of this shape as ONE kernel, 2 when they run it as the
 * precedence update followed by the placement (see above; for MACS the answer depends on the device's LDS).
 * on_bits != 0: tap_transition_bits / _first (the single kernels carry the one-word shadow: rows <= 64). */
int tap_transition_launches(const tap_ctx *ctx, const tap_env_desc *d, int n, int R, int rows, int on_bits);

/* tap_transition with the precedence update done on the bit shadow (tap_mask_step_bits).  The single kernels
 * carry the one-word shadow (rows <= 64); with the two-word shadow the step runs as its two launches. */
int tap_transition_bits(tap_ctx *ctx, const tap_env_desc *d, void *state, int n, int R, int rows,
                        int update_rows, const unsigned long long *bits_in, const float *static_,
                        int static_rows, const int64_t *ptr, const float *mask_in,
                        unsigned long long *bits_out, float *dyn_out, float *current_out,
                        float *mask_out, float *feature_out, float *ratio_out, int flags,
                        void *stream);

/* tap_transition_bits for the first step of an episode: the shadow is built from the fp32 tensor dyn_in
 * inside the launch (see tap_mask_step_first). */
int tap_transition_first(tap_ctx *ctx, const tap_env_desc *d, void *state, int n, int R, int rows,
                         int update_rows, const float *dyn_in, const float *static_, int static_rows,
                         const int64_t *ptr, const float *mask_in, unsigned long long *bits_out,
                         float *dyn_out, float *current_out, float *mask_out, float *feature_out,
                         float *ratio_out, int32_t *nonbinary_out, int flags, void *stream);

/* ---- trial placements: every selectable block scored without committing one ------------------- */

/* What would calc_ratio be if container b took column c next?  For all B containers and every selectable column in
 * one launch -- what the reference's greedy baseline generate_order_graph(..., find_order_type='best')
 * (generate.py:1242-1292: best_to_pack) gets from one deep copy of the target Container per selectable node.
 *   static_ / static_rows / nR   as tap_env_step_gather: the candidate of column c is static_[b, 1:1+D, c]
 *   mask        (B, nR) f32 or NULL = every column: the selectable columns (update_mask's current_mask)
 *   flags       TAP_T_FRESH: treat the blob as freshly reset (the fused stepper clears the container inside its first
 *               step, not before it); no other bit
 *   scores_out  (B, nR) f64 or NULL: for a column with mask != 0 the fp64 calc_ratio (tap_env_ratio's ratio64_out)
 *               container b would hold after tap_env_step_gather with ptr[b] = c; -1.0 when that step would raise
 *               an error bit (height overflow, count >= n_max, a side < 1 -- every real ratio is >= 0); -inf for a
 *               column with mask == 0
 *   best_out    (B,) int64 or NULL: the first column holding the row's maximum, compared in fp64 (the reference
 *               takes the first node with the strictly largest ratio, and a third of its steps have an exact fp64
 *               tie) = argmax(scores_out[b]); 0 where no column is selectable.  A NaN score (a block that fits
 *               nowhere in an empty container: 0 / 0) is never the best.
 * Read-only: no byte of the state blob changes, the sticky error words included.  No allocation, no host read, no
 * stream synchronisation: the call can be captured in a hipGraph.  One launch, one wavefront per container, its 64 / G
 * lane groups trying one column each per pass (k_trial_scores<D, G, HARD>; launch record key (25, D, G, HARD, MASK,
 * FRESH, 0)).  TAP_E_INVALID for a place-at descriptor; TAP_E_UNSUPPORTED outside the lane-per-cell LB_GREEDY kernels
 * (MACS / MUL, the legacy 'LB', more than 64 cells, a 3D side above 8): step those on a copy of the blob. */
int tap_env_trial_scores(tap_ctx *ctx, const tap_env_desc *d, const void *state, const float *static_,
                         int static_rows, int nR, const float *mask, int flags, double *scores_out,
                         int64_t *best_out, void *stream);

/* ---- the decoding head: masked softmax, pick and log-probability in one launch ------------------ */

enum {
    TAP_P_GREEDY = 1 /* take the most probable selectable column (model.py:370-372) instead of sampling */
};

/* The line between the pointer network and the step (model.py:359-372: softmax(logits + current_mask.log()), then
 * Categorical.sample() in a host loop that rejects unselectable picks + log_prob when training, torch.max + log when
 * not).  Per row b of nR columns:
 *   logits (B, nR) f32; mask (B, nR) f32: column c is selectable iff mask != 0 (update_mask's current_mask is 0 / 1, so
 *   logits + log(mask) is the logit there).  Logits on selectable columns must be finite.  Logits on unselectable
 *   columns never enter an arithmetic result, whatever they hold (NaN, +-inf: the reference's NaN + -inf poisons the row).
 *   All arithmetic in fp64, the order of summation free: m = max of the selectable logits, w_c = exp(l_c - m), S = sum w_c.
 *   u (B,) f32 in [0, 1), the caller's pre-drawn uniforms (sampling): t = (double)u * S; ptr = the first selectable column
 *   whose inclusive prefix sum of w, over the selectable columns in column order, is > t (strictly); the last
 *   selectable column when none is (t >= S).  An unselectable column is never returned: no rejection loop, no host read.
 *   flags TAP_P_GREEDY (u NULL): ptr = the first selectable column with l_c == m (the fp32 logits compare exactly).
 *   logp_out (B,) f32 = (float)((l_ptr - m) - log S); ptr_out (B,) int64.
 *   probs_out (B, nR) f32 or NULL: (float)(w_c / S), exactly 0 on unselectable columns -- what the backward reads.
 *   A row with no selectable column: ptr 0, logp NaN, probs all 0.
 * One launch, no allocation, no host read, no stream synchronisation (capturable in a hipGraph).  nR <= 64: a lane
 * group of G = 8 / 16 / 32 / 64 lanes per row (k_policy_pick<G, GREEDY>); above: one wavefront per row in 64-column
 * chunks (k_policy_pick_wide<GREEDY>).  Launch record key (26, 0, G, GREEDY, PROBS, 0, 0), G = 0 for the chunked form.
 * Checks, in this order, before anything touches the device: B < 0 or nR < 1 -> TAP_E_INVALID; B == 0 -> TAP_OK; a
 * null logits / mask / ptr_out / logp_out -> TAP_E_INVALID; TAP_P_GREEDY with u, or sampling without u ->
 * TAP_E_INVALID; unknown flag bits -> TAP_E_INVALID. */
int tap_policy_pick(tap_ctx *ctx, const float *logits, const float *mask, const float *u, int B, int nR,
                    int flags, int64_t *ptr_out, float *logp_out, float *probs_out /* or NULL */, void *stream);

/* The DRAW form: tap_policy_pick's sampling with the row's uniform computed INSIDE the launch, from the generator
 * tap_decoder_step_dropout defines -- Philox4x32-10, the same multipliers and key increments.  state: the int64[2]
 * (seed, episode) on the device; key (seed mod 2^32, seed >> 32); counter (env_offset + b, 0xFFFFFFFF, step, episode mod
 * 2^32) for row b of the call -- 0xFFFFFFFF is a hidden row no dropout launch can use, so one state feeds both without
 * overlap.  u = (float)(word0 >> 8) * 2^-24, exact in fp32 and in [0, 1); words 1 - 3 are unused.  Everything after u is
 * the sampling form's code in the sampling form's order: with u_out (B,) f32 (or NULL) fed back as u into tap_policy_pick
 * the outputs are the same bytes.  An env's pick depends on (seed, episode, step, env_offset + b) and its row alone: not
 * on B, G or the launch.  k_policy_pick_form<G, 2> / k_policy_pick_wide_form<2>, tap_policy_pick's geometry; launch
 * record key (26, 0, G, 2, PROBS, 0, 0).  Checks in tap_policy_pick's order, then a null state or one that is not 8-byte
 * aligned -> TAP_E_INVALID. */
int tap_policy_pick_draw(tap_ctx *ctx, const float *logits, const float *mask, const int64_t *state, uint32_t step,
                         uint32_t env_offset, int B, int nR, int64_t *ptr_out, float *logp_out,
                         float *probs_out /* or NULL */, float *u_out /* or NULL */, void *stream);

/* The GIVEN form: the log-probability of a caller's column (teacher forcing; old tours under new weights).  m and S as
 * tap_policy_pick computes them, then logp_out = (float)((l[ptr_in] - m) - log S) and probs_out as there.  A ptr_in
 * outside [0, nR) or on an unselectable column gives logp NaN (it is never used as an address); probs_out is still
 * written, and tap_policy_pick_backward writes zeros for such a row.  With ptr_in equal to what a sampling or greedy call
 * returned, logp and probs are that call's bytes.  k_policy_pick_form<G, 3> / k_policy_pick_wide_form<3>; launch record
 * key (26, 0, G, 3, PROBS, 0, 0).  Checks in tap_policy_pick's order (null logits / mask / logp_out), then a null ptr_in
 * -> TAP_E_INVALID. */
int tap_policy_pick_given(tap_ctx *ctx, const float *logits, const float *mask, const int64_t *ptr_in, int B, int nR,
                          float *logp_out, float *probs_out /* or NULL */, void *stream);

/* The backward of logp with respect to the logits (model.py:359-372 under autograd: log_softmax gathered at ptr), for
 * tap_policy_pick and both forms above (GIVEN: ptr = ptr_in):
 * dlogits_out[b, c] = -g[b] * probs[b, c] in fp32 for c != ptr[b], and the picked column = minus the fp64 sum of the
 * row's other results, rounded once (g (1 - p[ptr]) with a row that sums to zero within one rounding, as the true
 * gradient does); one thread per element; probs / ptr / logp as
 * tap_policy_pick wrote them, g (B,) f32 the gradient arriving at logp.  Rows whose logp is NaN (no selectable
 * column) are written as zeros whatever g holds.  The same argument checks (every buffer required). */
int tap_policy_pick_backward(tap_ctx *ctx, const float *probs, const int64_t *ptr, const float *logp,
                             const float *g, int B, int nR, float *dlogits_out, void *stream);

/* ---- the dynamic encoder on the bit shadow: from bits to hidden in one launch ------------------- */

/* The reference's first use of `dynamic` after every step (model.py:380: dynamic_hidden = self.dynamic_encoder(dynamic), an
 * nn.Conv1d(rows, H, kernel_size=1)) computed from the shadow, so that a loop on a stepper without the fp32 expansion
 * (tap_stepper_buffers.dyn NULL) never writes or reads that tensor.  A 1x1 convolution of a 0/1 tensor needs no
 * multiplication:
 *   bits (B, tap_bits_words(rows, nR)) the shadow in tap_dyn_bits' layout: word c of plane p holds rows 64p .. 64p + 63 of
 *   column c.  Bits at positions >= rows are IGNORED, whatever they hold.
 *   weight (H, rows) f32 row-major = Conv1d.weight (H, rows, 1); bias (H,) f32 or NULL = zeros.
 *   out[b, h, c] (B, H, nR) f32 = the fp32 sum that starts at bias[h] (+0.0f without a bias) and adds, one fp32 addition
 *   per row in ASCENDING row order (plane 0 before plane 1), W[h, r] for a set row and +0.0f for an unset one -- the same
 *   value as adding the set rows only, up to the sign of a zero.  No multiplication, no reassociation, no contraction: the
 *   result is reproducible bit for bit and equals the sequential fp32 sum of a model that follows the same order.
 * Shapes: every window with a shadow (tap_bits_words(rows, nR) > 0: rows <= 128, nR % 4 == 0, nR <= 256) and
 * 1 <= H <= 1024; anything else -> TAP_E_UNSUPPORTED.  bits 8-byte aligned (any offset view of a shadow), out 16-byte.
 * One launch, no allocation, no host read, no stream synchronisation (capturable in a hipGraph).  k_encode_bits<HPL>: a
 * wavefront per (env, column) with lanes along the hidden rows (HPL = 1 or 2 rows per lane), a scalar loop over the
 * column's set bits, one LDS read and one addition per set row, the results transposed through an LDS tile and stored as
 * float4s, consecutive threads consecutive 16-byte pieces (encode.hip).  Launch record key (27, 0, HPL, PLANES, BIAS, 0, 0).
 * Checks, in tap_policy_pick's order, before anything touches the device: B < 0 or nR / rows / H < 1 -> TAP_E_INVALID;
 * B == 0 -> TAP_OK; a null bits / weight / out -> TAP_E_INVALID; a shape outside the list above -> TAP_E_UNSUPPORTED; a
 * misaligned bits / out -> TAP_E_INVALID. */
int tap_encode_bits(tap_ctx *ctx, const unsigned long long *bits, int B, int nR, int rows, int H,
                    const float *weight, const float *bias /* or NULL */, float *out, void *stream);

/* The backward of tap_encode_bits with respect to weight and bias (the bits have no gradient):
 *   dweight[h, r] (H, rows) = sum over b, c of g[b, h, c] * bit[b, r, c];  dbias[h] (H,) or NULL = sum over b, c of g[b, h, c];
 *   g (B, H, nR) f32, 16-byte aligned, the gradient arriving at out.  fp32 accumulators; the summation order is fixed by
 *   the shape alone (columns in order inside an env, envs in order inside a slice, slices in order), NO atomics: two
 *   calls on the same inputs give the same bytes.  Two launches (per-slice partials into `scratch`, then their sum), no
 *   allocation inside: scratch (floats: 4-byte aligned) holds at least tap_encode_bits_backward_scratch(B, nR, rows, H)
 *   bytes, a smaller scratch_bytes (or a null scratch) -> TAP_E_INVALID.  The forward's checks in the forward's order
 *   (bits / g / dweight required, then the shape, then the scratch, then the alignment); B == 0 -> TAP_OK with nothing
 *   written.
 * Launch record key (27, 0, 0, PLANES, DBIAS, 1, 0), one count per call. */
int tap_encode_bits_backward(tap_ctx *ctx, const unsigned long long *bits, const float *g, int B, int nR, int rows, int H,
                             float *dweight, float *dbias /* or NULL */, void *scratch, size_t scratch_bytes, void *stream);
/* bytes of scratch the backward needs for this shape (0 for a shape the entry refuses) */
size_t tap_encode_bits_backward_scratch(int B, int nR, int rows, int H);
/* The launch geometry of tap_encode_bits (backward = 0) or tap_encode_bits_backward (backward != 0) for this shape, from
 * the function the launcher itself calls: host only, no context, no GPU code, like tap_bits_words.  Forward: out =
 * (consecutive envs per workgroup, grid x = runs of envs, grid y = hidden chunks, bytes of dynamic LDS).  Backward: out =
 * (envs per slice, slices, hidden chunks, hidden rows per chunk); the scratch above is slices * H * (rows + 1) floats.
 * TAP_OK; a null out -> TAP_E_INVALID; B, nR, rows or H < 1 -> TAP_E_INVALID and a shape the entries refuse ->
 * TAP_E_UNSUPPORTED, both with out = zeros (as the scratch query answers 0). */
int tap_encode_bits_geometry(int B, int nR, int rows, int H, int backward, int32_t out[4]);

/* ---- the pointer network on the bit shadow: glimpse and logits in one launch -------------------- */

/* The line between the dynamic encoder and the decoding head (model.py:356-358: probs, last_hh = self.pointer(static_hidden,
 * dynamic_hidden, decoder_hidden, last_hh); classes Attention and Pointer, model.py:38-138) after its GRU step, with
 * everything that does not depend on the step folded out.  He / Hd the encoder / decoder hidden sizes, Wa =
 * encoder_attn.W[0] (Hd, 2 He + Hd), Wp = W[0] (Hd, 4 He), We / be the dynamic encoder's conv.weight[:, :, 0] / conv.bias.
 * The caller prepares, in differentiable host code: Ws = [Wa[:, :He]; Wp[:, :He]; Wp[:, 2He:3He]] and Wd = [Wa[:, He:2He];
 * Wp[:, He:2He]; Wp[:, 3He:4He]] (3 Hd, He); proj = Ws . static_hidden once per EPISODE; M = Wd . We (3 Hd, rows), k = Wd . be
 * (3 Hd,); q = rnn_out . Wa[:, 2He:]^T (B, Hd) per step.  Per env b and column c, all in fp32:
 *   U[x, c]   = proj[b, x, c] + (k[x] + the M[x, r] of the rows r set in column c, added to k in ASCENDING row order)
 *   s[c]      = sum_j va[j] tanh(U[j, c] + q[b, j])
 *   attn      = softmax_c(s)  over ALL nR columns, unmasked, as the reference's Attention is
 *   t[j]      = sum_c attn[c] U[2 Hd + j, c]
 *   logits[c] = sum_j vp[j] tanh(U[Hd + j, c] + t[j])
 * which equals the reference's arithmetic in exact arithmetic (the context is a convex combination of columns, so W's
 * action on it is the same combination of W's action on the columns).
 *   proj (B, 3, nR, Hd) f32, SEGMENT-major and hidden fastest: proj[b, x, c] above is element [b][x / Hd][c][x % Hd] -- a
 *   wavefront reads 256 contiguous bytes per load.  bits (B, tap_bits_words(rows, nR)) the shadow in tap_dyn_bits' layout;
 *   bits at positions >= rows are IGNORED.  M (3 Hd, rows) row-major, k (3 Hd,), q (B, Hd), va / vp (Hd,).
 *   logits_out (B, nR), attn_out (B, nR), t_out (B, Hd): attn and t are what the backward reads.
 * The order of every sum is fixed by the shape (a lane's hidden rows in order, an xor butterfly over the 64 lanes, the
 * hidden chunks in order; the columns of a wavefront in order, the four wavefronts in order): two calls give the same
 * bytes.  No atomics, no contraction.  One launch, no allocation, no host read, no stream synchronisation (capturable in a
 * hipGraph).  k_pointer_scores<HPL> (pointer.hip): a workgroup per run of consecutive envs, a wavefront per column, lanes
 * along the hidden rows (HPL = 1 or 2 rows per lane), the phases s / t / logits as outer loops so that each third of proj
 * is read once and the LDS holds one chunk of one third of M.  Launch record key (28, 0, HPL, PLANES, CHUNKS, 0, 0), CHUNKS
 * = Hd / (64 HPL).
 * Shapes: every window with a shadow (rows <= 128, nR % 4 == 0, nR <= 256) and Hd 64, 128 or 256; anything else ->
 * TAP_E_UNSUPPORTED.  Checks, in tap_policy_pick's order: B < 0 or nR / rows / Hd < 1 -> TAP_E_INVALID; B == 0 -> TAP_OK; a
 * null buffer -> TAP_E_INVALID; a shape outside the list -> TAP_E_UNSUPPORTED; a misaligned buffer (bits 8 bytes, floats
 * 4) -> TAP_E_INVALID. */
int tap_pointer_scores(tap_ctx *ctx, const float *proj, const unsigned long long *bits, int B, int nR, int rows, int Hd,
                       const float *M, const float *k, const float *q, const float *va, const float *vp,
                       float *logits_out, float *attn_out, float *t_out, void *stream);

/* The backward of tap_pointer_scores: g (B, nR) the gradient arriving at logits, attn / t as the forward wrote them, the
 * forward's inputs; U, A = U + q and G = U + t are recomputed.  Writes
 *   dU_out (B, 3 Hd, nR) f32, columns fastest -- dproj is this tensor (read through the transposed view), and
 *   tap_encode_bits_backward with g = dU_out and H = 3 Hd gives dM and dk --; dq_out (B, Hd); dva_out, dvp_out (Hd,).
 * dva / dvp go through one partial per workgroup in `scratch` (at least tap_pointer_scores_backward_scratch(B, nR, rows,
 * Hd) bytes; a smaller scratch_bytes or a null scratch -> TAP_E_INVALID) and a second launch that adds them in workgroup
 * order: no atomics, two calls give the same bytes.  The forward's checks in the forward's order (every buffer
 * required), then the scratch, then the alignment (dU_out leaves as float4s through an LDS tile: 16 bytes); B == 0 ->
 * TAP_OK with nothing written.
 * Launch record key (28, 0, HPL, PLANES, CHUNKS, 1, 0), one count per call. */
int tap_pointer_scores_backward(tap_ctx *ctx, const float *proj, const unsigned long long *bits, int B, int nR, int rows,
                                int Hd, const float *M, const float *k, const float *q, const float *va, const float *vp,
                                const float *attn, const float *t, const float *g, float *dU_out, float *dq_out,
                                float *dva_out, float *dvp_out, void *scratch, size_t scratch_bytes, void *stream);
/* bytes of scratch the backward needs for this shape (0 for a shape the entry refuses) */
size_t tap_pointer_scores_backward_scratch(int B, int nR, int rows, int Hd);

/* tap_pointer_scores with the static term of U computed from the S rows of `static` that the static encoder sees, in
 * place of proj: static_hidden = Es . xs + bs is a 1x1 convolution, so with G = Ws . Es (3 Hd, S) and g = Ws . bs (3 Hd,),
 * prepared by the caller in differentiable host code from the parameters alone, per env b, column c and hidden row x in
 * fp32:
 *   P[x, c]   = g[x], then fmaf(G[x, i], xs[b, i, c], .) for i = 0 .. S - 1 (ascending, as tap_critic_value orders it)
 *   U[x, c]   = P[x, c] + (k[x] + the M[x, r] of the rows r set in column c, ascending, plane 0 before plane 1)
 *   s, attn, t, logits: tap_pointer_scores' lines on this U
 * -- tap_pointer_scores' contract with proj := P, every order of summation and the assignment of columns to wavefronts
 * included: given a proj that equals P bit for bit both entries write the same bytes.  No proj, no static_hidden: an
 * episode keeps xs (B S nR floats) where it kept 3 Hd nR floats per env.
 *   xs (B, S, nR) f32 contiguous; G (3 Hd, S) row-major; g (3 Hd,) -- k and g stay separate arguments; the rest as
 *   tap_pointer_scores takes it.
 * k_pointer_scores<HPL, SS> (pointer.hip), tap_pointer_scores' kernel with another source for the static term: SS = S
 * for S = 2, 3, 4 (a lane's HPL S values of G in registers), SS = 0 for S = 1 and 5 .. 8 (an LDS copy [i][hidden] of the
 * chunk's G).  xs[b, :, c] is wave-uniform.  One launch, no allocation, no host read, capturable in a hipGraph.
 * Launch record key (28, 0, HPL, PLANES, CHUNKS, 0, S).
 * Shapes: tap_pointer_scores' and 1 <= S <= 8.  Checks, in tap_pointer_scores' order: B < 0 or nR / rows / Hd / S < 1 ->
 * TAP_E_INVALID; B == 0 -> TAP_OK; a null buffer -> TAP_E_INVALID; a shape outside the list or S > 8 ->
 * TAP_E_UNSUPPORTED; a misaligned buffer (bits 8 bytes, floats 4) -> TAP_E_INVALID. */
int tap_pointer_scores_static(tap_ctx *ctx, const float *xs, const unsigned long long *bits, int B, int nR, int rows, int Hd,
                              int S, const float *G, const float *g, const float *M, const float *k, const float *q,
                              const float *va, const float *vp, float *logits_out, float *attn_out, float *t_out, void *stream);

/* The backward of tap_pointer_scores_static: tap_pointer_scores_backward with P recomputed from xs, G and g.  Writes
 * dU_out (B, 3 Hd, nR), dq_out (B, Hd), dva_out, dvp_out (Hd,) as that entry does; from dU the caller gets dM and the bias
 * sum (tap_encode_bits_backward with H = 3 Hd: the sum is dk and dg alike) and dG[x, i] = sum over (b, c) of dU[b, x, c]
 * xs[b, i, c].  xs carries no gradient.  Given a proj that equals P bit for bit, dU and dq are tap_pointer_scores_backward's
 * bytes; dva / dvp are sums of one partial per workgroup and may differ in the last bits where the LDS copy of G (SS = 0)
 * leaves room for fewer envs per workgroup.  scratch: at least tap_pointer_scores_static_backward_scratch(B, nR, rows, Hd,
 * S) bytes.  The forward's checks in the forward's order (every buffer required), then the scratch, then the alignment
 * (dU_out 16 bytes); B == 0 -> TAP_OK with nothing written.
 * Launch record key (28, 0, HPL, PLANES, CHUNKS, 1, S), one count per call. */
int tap_pointer_scores_static_backward(tap_ctx *ctx, const float *xs, const unsigned long long *bits, int B, int nR, int rows,
                                       int Hd, int S, const float *G, const float *g, const float *M, const float *k,
                                       const float *q, const float *va, const float *vp, const float *attn, const float *t,
                                       const float *grad, float *dU_out, float *dq_out, float *dva_out, float *dvp_out,
                                       void *scratch, size_t scratch_bytes, void *stream);
/* bytes of scratch the backward needs for this shape (0 for a shape the entry refuses) */
size_t tap_pointer_scores_static_backward_scratch(int B, int nR, int rows, int Hd, int S);
/* The launch geometry of the four pointer entries for this shape, from the function the launchers themselves call: host
 * only, no context, no GPU code, like tap_bits_words.  S = 0: tap_pointer_scores / _backward; S = 1 .. 8: the static-rows
 * form, and with backward = 0 tap_pointer_pick_static too (its epilogue needs no LDS of its own); backward != 0: the backward.  out = (consecutive envs per workgroup -- max(1, B / 1024), halved while the dynamic
 * LDS exceeds 60 KB --, workgroups = ceil(B / envs per workgroup), bytes of dynamic LDS, columns per pass of the backward's
 * dU tile (0 forward)); the backward's scratch is workgroups * 2 * Hd floats.  TAP_OK; a null out -> TAP_E_INVALID; B, nR,
 * rows or Hd < 1 or S < 0 -> TAP_E_INVALID and a shape the entries refuse -> TAP_E_UNSUPPORTED, both with out = zeros (as
 * the scratch queries answer 0). */
int tap_pointer_scores_geometry(int B, int nR, int rows, int Hd, int S, int backward, int32_t out[4]);

enum {
    TAP_PICK_GREEDY = 1, /* the head's greedy form: tap_policy_pick with TAP_P_GREEDY */
    TAP_PICK_DRAW = 2    /* the head's DRAW form: tap_policy_pick_draw */
};

/* Scores and pick in ONE launch, for inference on windows whose static rows change every step (the rolling loop):
 * tap_pointer_scores_static followed by the decoding head, with the logits never leaving the LDS.  No attn, no t, no
 * gradient.
 *   xs: env b's S rows start at xs + b * xs_env_stride floats; the rows are nR floats apart and contiguous (xs_env_stride
 *   >= S nR) -- static[:, 1:, :] of a (B, 1 + S, nR) window is passed as the view it is, xs_env_stride = (1 + S) nR.
 *   bits, B, nR, rows, Hd, S, G, g, M, k, q, va, vp: tap_pointer_scores_static's.
 *   mask (B, nR) f32: the stepper's current_mask, column c selectable iff mask != 0 (tap_policy_pick's).
 *   form: TAP_PICK_GREEDY, or TAP_PICK_DRAW with state / step / env_offset exactly as tap_policy_pick_draw takes them
 *   (state is not read under TAP_PICK_GREEDY and may be NULL).
 *   ptr_out (B,) int64, logp_out (B,) f32; logits_out (B, nR) f32 or NULL.
 * Byte contract: logits_out, when given, holds the bytes tap_pointer_scores_static writes for the same inputs (xs made
 * contiguous), and ptr_out / logp_out hold the bytes tap_policy_pick with TAP_P_GREEDY / tap_policy_pick_draw writes when
 * fed those logits and this mask -- for every supported nR, whichever of the head's two geometries the stand-alone launch
 * takes.  A row without a selectable column: ptr 0, logp NaN.
 * k_pointer_pick<HPL, SS, FORM> (pointer.hip): k_pointer_scores<HPL, SS>'s three phases on tap_pointer_scores_geometry(B, nR,
 * rows, Hd, S, 0)'s geometry -- the same LDS, the same orders of summation --; then, where that kernel stores the LDS row of
 * logits, one wavefront per env of the workgroup's run walks it in 64-column chunks: the head's chunked form (max pass,
 * fp64 weights, the 64-lane scan with the running prefix, DRAW's second pass; tap_pick.h holds the code both units run).
 * On rows of at most 64 columns the lane-group form agrees with it bit for bit: its scan's extra steps add lanes that
 * hold 0.0, and a lane's partial sums are the same operations.  One launch, no allocation, no host read, no stream
 * synchronisation (capturable in a hipGraph); no atomics: two calls give the same bytes.
 * Launch record key (28, FORM, HPL, PLANES, CHUNKS, 0, S), FORM = 1 (greedy) or 2 (DRAW) where the entries above have 0.
 * Checks, in tap_pointer_scores_static's order: B < 0 or nR / rows / Hd / S < 1, or a form that is neither ->
 * TAP_E_INVALID; B == 0 -> TAP_OK; a null buffer (mask, ptr_out and logp_out among them; not logits_out) ->
 * TAP_E_INVALID; TAP_PICK_DRAW with a null state or one that is not 8-byte aligned -> TAP_E_INVALID; xs_env_stride <
 * S nR -> TAP_E_INVALID; a shape outside tap_pointer_scores_static's list -> TAP_E_UNSUPPORTED; a misaligned buffer
 * (bits and ptr_out 8 bytes, floats 4) -> TAP_E_INVALID. */
int tap_pointer_pick_static(tap_ctx *ctx, const float *xs, size_t xs_env_stride, const unsigned long long *bits, int B, int nR,
                            int rows, int Hd, int S, const float *G, const float *g, const float *M, const float *k,
                            const float *q, const float *va, const float *vp, const float *mask, int form,
                            const int64_t *state, uint32_t step, uint32_t env_offset, int64_t *ptr_out, float *logp_out,
                            float *logits_out /* or NULL */, void *stream);

/* The state critic's value estimate in ONE launch from the critic's static input and the bit shadow (critic.hip): the
 * reference's realCritic (trainer.py:18-94) after its GRU step.  With Es, bs / Ed, bd the static / dynamic encoder's
 * conv, W = attention.W[0] = [Was | Wad | Waq] (H, 3H), v = attention.v[0, 0], F1, f1 = fc.0 and w2, b2 = fc.2 the caller
 * folds, from the parameters alone (tools.StateCritic.fold):
 *   G = [Was Es ; Waq Es ; F1 Es] (3H, S), g = [Was bs + Wad bd ; Waq bs ; F1 bs + f1] (3H,), M = Wad Ed (H, rows),
 *   q0 = Waq . rnn_out (B, H) -- or ONE row for the whole batch, q0_stride 0.
 * Per env b, in fp32, n = blocks:
 *   U[j, c]    = g[j] + the M[j, r] of the rows r set in column c (ASCENDING, plane 0 before plane 1), then
 *                fmaf(G[j, i], x[b, i, c], .) for i = 0 .. S - 1
 *   for i in 0 .. n - 1:
 *     s[c]       = sum_j v[j] tanhf(U[j, c] + q_i[j]);  p_i = softmax_c(s) over ALL nR columns, unmasked
 *     xbar_i[k]  = sum_c p_i[c] x[b, k, c]
 *     q_{i+1}[j] = g[H + j], then fmaf(G[H + j, k], xbar_i[k], .) for k ascending       (not after the last block)
 *   z[j]       = g[2H + j], then fmaf(G[2H + j, k], xbar_{n-1}[k], .)
 *   value      = b2 + sum_j w2[j] max(z[j], 0)
 * which equals the reference's arithmetic in exact arithmetic: every context is static_hidden . p with sum p = 1, i.e.
 * Es (x . p) + bs.
 *   x (B, S, nR) f32; bits (B, tap_bits_words(rows, nR)) the shadow in tap_dyn_bits' layout, bits at positions >= rows are
 *   IGNORED; an all-zero shadow gives U without M entering, whatever M holds; G, M row-major; q0 (B, H) with q0_stride = H
 *   or (H,) with q0_stride = 0; b2 a device pointer to one float.
 *   value_out (B,), z_out (B, H), p_out (B, n, nR), xbar_out (B, n, S), q_out (B, n, H) with q_out[:, 0] = q0: what the
 *   backward reads.
 * The order of every sum is fixed by the shape (a lane's hidden rows in order, an xor butterfly over the 64 lanes, the
 * 64-row slabs in order where M is staged by slabs; a lane's columns in order, then the butterfly): two calls give the
 * same bytes.  No atomics, no contraction beyond the fmafs above.  One launch, no allocation, no host read, no stream
 * synchronisation (capturable in a hipGraph).  k_critic_value<HPL>: a wavefront per env, four envs per workgroup, lanes
 * along the hidden rows (HPL = H / 64 rows per lane).  Launch record key (31, RES, HPL, PLANES, MALL, 0, 0).
 * Shapes: every window with a shadow (rows <= 128, nR % 4 == 0, nR <= 256), H 64, 128 or 256, S <= 8, blocks <= 8,
 * q0_stride 0 or H; anything else -> TAP_E_UNSUPPORTED.  Checks, in tap_pointer_scores' order: B < 0 or nR / rows / H / S /
 * blocks < 1 -> TAP_E_INVALID; B == 0 -> TAP_OK; a null buffer -> TAP_E_INVALID; a shape outside the list ->
 * TAP_E_UNSUPPORTED; a misaligned buffer (bits 8 bytes, floats 4) -> TAP_E_INVALID. */
int tap_critic_value(tap_ctx *ctx, const float *x, const unsigned long long *bits, int B, int nR, int rows, int H, int S,
                     int blocks, const float *G, const float *g, const float *M, const float *q0, int q0_stride,
                     const float *v, const float *w2, const float *b2, float *value_out, float *z_out, float *p_out,
                     float *xbar_out, float *q_out, void *stream);

/* The backward of tap_critic_value from dz (B, H) = g_value w2 [z > 0] (the caller's element-wise product): q and p as
 * the forward wrote them, the forward's inputs; U and the tanh arguments are recomputed.  For i = n - 1 down to 0:
 * dxbar_i = G2^T dz for the last block, else G1^T dq_{i+1}; dp[c] = sum_k dxbar_i[k] x[k, c]; ds = p_i (dp - sum p_i dp);
 * dA[j, c] = ds[c] v[j] (1 - tanh^2); dU += dA; dq_i[j] = sum_c dA[j, c]; dv[j] += sum_c ds[c] tanh(.).  Writes
 *   dU_out (B, H, nR) f32, columns fastest -- tap_encode_bits_backward with g = dU_out gives dM and the bias sum --;
 *   dq_out (B, n, H); dv_out (H,).
 * dv goes through one partial per workgroup in `scratch` (at least tap_critic_value_backward_scratch(...) bytes; a
 * smaller scratch_bytes or a null scratch -> TAP_E_INVALID) and a second launch that adds them in workgroup order: no
 * atomics, two calls give the same bytes.  The forward's checks in the forward's order (every buffer required), then the
 * scratch, then the alignment (dU_out leaves as float4s: 16 bytes); B == 0 -> TAP_OK with nothing written.
 * Launch record key (31, RES, HPL, PLANES, MALL, 1, 0), one count per call. */
int tap_critic_value_backward(tap_ctx *ctx, const float *x, const unsigned long long *bits, int B, int nR, int rows, int H,
                              int S, int blocks, const float *G, const float *g, const float *M, const float *v,
                              const float *q, const float *p, const float *dz, float *dU_out, float *dq_out,
                              float *dv_out, void *scratch, size_t scratch_bytes, void *stream);
/* bytes of scratch the backward needs for this shape (0 for a shape the entry refuses) */
size_t tap_critic_value_backward_scratch(int B, int nR, int rows, int H, int S, int blocks);

/* The decoder side of a decoding step in ONE launch (model.py:347-354 and the GRU step of 108-115, then the decoder's
 * columns of the attention's W): from the stepper's decoder buffers and last_hh to the new hidden state and the q that
 * tap_pointer_scores takes.  The decoder's encoders are 1x1 convolutions, so the caller folds them into the GRU's input
 * weights once per episode (tools.Pointer.fold_decoder): P (3 Hd, K) and c (3 Hd,), K = Ks + Kd, gate order r, z, n as
 * nn.GRU lays weight_ih_l0 out.  Per env, with xs (Ks) the chosen block's sides, xd (Kd) the container feature and h (Hd)
 * the previous hidden state:
 *   gi = P . [xs ; xd] + c        gh = w_hh . h + b_hh          (w_hh (3 Hd, Hd), b_hh (3 Hd,): weight_hh_l0, bias_hh_l0)
 *   r = sigmoid(gi_r + gh_r)      z = sigmoid(gi_z + gh_z)      n = tanh(gi_n + r gh_n)
 *   h' = (1 - z) n + z h          q = wq . h'                   (wq (Hd, Hd) = encoder_attn.W[0][:, 2 He:])
 * fp32 throughout, sigmoid(x) = 1 / (1 + expf(-x)).  Every sum is one chain of fmaf in ascending term order: gi_g[j] starts
 * from c[g Hd + j] and takes the K inputs, static columns first; gh_g[j] starts from b_hh[g Hd + j] and takes the Hd hidden
 * terms; q[j] starts from 0 and takes the Hd terms of h'.  The products r gh_n, (1 - z) n and z h are rounded before they
 * are added (no contraction).  No atomics, no cross-lane sums: two calls give the same bytes, and an env's result does not
 * depend on the batch around it.
 *   xs (B, Ks) and xd (B, Kd) are two buffers of their own (a stepper's flat decoder buffer holds the feature part
 *   first, then the block part: no concatenation is needed); xs may be null iff Ks == 0, xd iff Kd == 0.  h (B, Hd), or
 *   NULL for the zero state of step 0: gh is then exactly b_hh and w_hh is not read.  h_out, q_out (B, Hd).  gates_out
 *   (B, 4, Hd) = r, z, n, gh_n -- what the backward reads -- or NULL: written only when given.
 * One launch, no allocation, no host read, no stream synchronisation (capturable in a hipGraph).  k_decoder_step
 * (decoder.hip): a workgroup per 16 consecutive envs with their h and h' rows in the LDS, a wavefront per 4 of them, a lane
 * per hidden row and its three gates; the weights pass through the LDS in blocks of 64 hidden rows x 32 terms, the hidden
 * chunk outermost; one barrier completes h' of the tile before q.  Launch record key (29, 0, TE, Hd / 64, H, 0, 0): TE = 16
 * envs per workgroup, H 1 = h given.
 * Shapes: Hd 64, 128 or 256 and 1 <= Ks + Kd <= Hd + 16; anything else -> TAP_E_UNSUPPORTED.  Checks, in
 * tap_pointer_scores' order: B, Ks or Kd < 0 or Hd < 1 -> TAP_E_INVALID; B == 0 -> TAP_OK; a null required buffer ->
 * TAP_E_INVALID; a shape outside the list -> TAP_E_UNSUPPORTED; a buffer that is not 4-byte aligned -> TAP_E_INVALID (every
 * load and store of the kernel's is 4 bytes wide: xs / xd are views into the stepper's flat buffer). */
int tap_decoder_step(tap_ctx *ctx, const float *xs, int Ks, const float *xd, int Kd, const float *h, int B, int Hd,
                     const float *P, const float *c, const float *w_hh, const float *b_hh, const float *wq,
                     float *h_out, float *q_out, float *gates_out, void *stream);

/* The element-wise part of tap_decoder_step's backward, one launch: from gates (B, 4, Hd) as the forward wrote them, h
 * (or NULL, as the forward had it) and g_h (B, Hd), the gradient arriving at h' (the caller has added wq^T . dq to it):
 *   da_n = g_h (1 - z) (1 - n^2)      da_r = da_n gh_n r (1 - r)      da_z = g_h (h - n) z (1 - z)
 *   dgi_out (B, 3 Hd) = [da_r | da_z | da_n];  dghn_out (B, Hd) = da_n r (the n gate's hidden side; the r and z parts of
 *   dgh equal those of dgi);  dh_carry_out (B, Hd) = g_h z.
 * The sums over the batch (dP, dc, dw_hh, db_hh, dwq) and dh = carry + dgh . w_hh are the caller's GEMMs.  Element-wise:
 * two calls give the same bytes.  Checks: B < 0 or Hd < 1 -> TAP_E_INVALID; B == 0 -> TAP_OK; a null buffer (h excepted)
 * -> TAP_E_INVALID; Hd not 64, 128 or 256 -> TAP_E_UNSUPPORTED; 4-byte alignment.  Launch record key (29, 0, TE, Hd / 64, H,
 * 1, 0). */
int tap_decoder_step_backward(tap_ctx *ctx, int B, int Hd, const float *gates, const float *h, const float *g_h,
                              float *dgi_out, float *dghn_out, float *dh_carry_out, void *stream);

/* tap_decoder_step with the reference's 3D dynamic_decoder in front of it, in the SAME launch: a HeightmapEncoder
 * (model.py:21-35) has two leaky-ReLUs and does not fold into the GRU's input weights, but it is small.  conv1 and conv2 have
 * kernel size 1 and stride 2, and conv3's kernel covers what is left of the map, so the output is 1 x 1 and only the cells
 * (4i, 4j) of each plane are read.  With hm (B, C, W, L) the stepper's decoder_dynamic, nw = ceil(W / 4), nl = ceil(L / 4),
 * Np = nw nl, position p = i nl + j, C1 = m / 4, C2 = m / 2 and m the encoder's hidden size, per env b:
 *   a1[p, o] = leaky(b1[o] + sum_c  w1[o, c]  hm[b, c, 4i, 4j])      o < C1, c ascending       (w1 (C1, C), conv1.weight)
 *   a2[p, o] = leaky(b2[o] + sum_c1 w2[o, c1] a1[p, c1])             o < C2, c1 ascending      (w2 (C2, C1), conv2.weight)
 *   enc[o]   = b3[o] + sum_t w3[o, t] a2flat[t]                      o < m, t = c2 Np + p ascending
 *   leaky(x) = x > 0 ? x : 0.01f x
 * t is conv3.weight's own memory order: (m, C2, nw, nl) read as (m, C2 Np).  After that the step is tap_decoder_step's
 * contract, word for word, with xd = enc and Kd = m: gi = P . [xs ; enc] + c with P (3 Hd, Ks + m), the GRU cell, h' and
 * q = wq . h'; the same sum orders, the products rounded in the same places, h == NULL the zero state.  fp32 throughout; every
 * sum of the encoder stage is one chain of fmaf in the ascending order above, starting from its bias.  No atomics, no sum
 * depends on the batch or the tile: two calls give the same bytes, and an env's result does not depend on the envs around
 * it.
 *   xs (B, Ks), null iff Ks == 0.  h (B, Hd) or NULL.  h_out, q_out (B, Hd); gates_out (B, 4, Hd) = r, z, n, gh_n or NULL;
 *   enc_out (B, m) or NULL -- what the caller's backward of the encoder starts from.  Both optional outputs are written
 *   only when given.
 * One launch, no allocation, no host read, no stream synchronisation (capturable in a hipGraph).  k_decoder_step_hm
 * (heightmap.hip): tap_decoder_step's geometry -- a workgroup per 16 consecutive envs, a wavefront per 4 of them, a lane per
 * output row, weights through the LDS in 64 row x 32 term blocks.  The encoder stage runs first on the tile and leaves a2
 * (16 x C2 Np) and then enc (16 x m) in the LDS; the input product takes its dynamic terms from that enc tile.  Envs past B
 * in the last tile read nothing and write nothing.  Launch record key (30, C, Np, Hd / 64, H, 0, 0), H 1 = h given.
 * Shapes: Hd 64, 128 or 256; m = Hd / 2 or Hd; C 1, 2 or 4; 1 <= W, L <= 12 (Np <= 9); 0 <= Ks <= 16 and Ks + m <= Hd + 16;
 * anything else -> TAP_E_UNSUPPORTED.  Checks, in tap_decoder_step's order: B or Ks < 0, or C, W, L, Hd or m < 1 ->
 * TAP_E_INVALID; B == 0 -> TAP_OK; a null required buffer -> TAP_E_INVALID; a shape outside the list -> TAP_E_UNSUPPORTED; a
 * buffer that is not 4-byte aligned -> TAP_E_INVALID.  The backward is tap_decoder_step_backward from gates_out plus the
 * caller's matmuls (rollout.decoder_step_heightmap). */
int tap_decoder_step_hm(tap_ctx *ctx, const float *xs, int Ks, const float *hm, int C, int W, int L, const float *h, int B,
                        int Hd, int m, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                        const float *b3, const float *P, const float *c, const float *w_hh, const float *b_hh,
                        const float *wq, float *h_out, float *q_out, float *gates_out, float *enc_out, void *stream);

/* tap_decoder_step with the pointer's two dropouts (model.py:112-115: drop_rnn on the GRU's output, drop_hh on last_hh)
 * inside the launch, for training.  Both are element-wise masks on h'; the random source is a counter-based generator, so
 * the masks are the same bytes on every call, need no host value, change on every replay of a captured graph and can be
 * recomputed anywhere (rollout.dropout_keep_words is the torch form, tests/step_dropout_model.py the numpy one).
 *   Generator: Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.
 *   For env b of the call, hidden row j:  counter = (env_offset + b, j, step, episode mod 2^32),  key = (seed mod 2^32,
 *   seed >> 32), with (seed, episode) = state[0], state[1] -- an int64[2] ON THE DEVICE, read by the launch.  Output word 0
 *   decides drop_rnn, word 1 drop_hh; words 2 and 3 are unused.
 *   Keep iff word >= thr, thr = min(2^32 - 1, round(p 2^32)) computed by the caller, one per mask.  A kept element is
 *   h' s with s = float32(1 / (1 - p)), a dropped one +0.0f.  thr = 0, s = 1 keeps everything: the bytes of tap_decoder_step.
 *   An env's masks depend on (seed, episode, step, env_offset + b, j) and on nothing else.
 * h_out (B, Hd) = drop_hh(h'); q_out = wq . drop_rnn(h') in tap_decoder_step's order; gates_out (B, 4, Hd) or NULL as
 * tap_decoder_step writes it (r, z, n, gh_n of the step before any mask); rnn_out (B, Hd) = drop_rnn(h') or NULL -- the
 * backward's dwq needs it; keep_out (B, 2, Hd / 64) int64: plane 0 drop_rnn, plane 1 drop_hh, bit j mod 64 of word j / 64
 * set iff row j is kept (one wavefront ballot per word, stored by one lane with an ordinary vector store).  Everything
 * else -- geometry, sum orders, shapes, the order of the checks -- is tap_decoder_step's; a null state or keep_out ->
 * TAP_E_INVALID with the other null buffers, and both must be 8-byte aligned.  Launch record key (29, 0, TE, Hd / 64, H, 2,
 * 0): a dropout launch never records variant 0. */
int tap_decoder_step_dropout(tap_ctx *ctx, const float *xs, int Ks, const float *xd, int Kd, const float *h, int B, int Hd,
                             const float *P, const float *c, const float *w_hh, const float *b_hh, const float *wq,
                             const int64_t *state, uint32_t step, uint32_t env_offset, uint32_t thr_rnn, uint32_t thr_hh,
                             float s_rnn, float s_hh, float *h_out, float *q_out, float *gates_out, float *rnn_out,
                             int64_t *keep_out, void *stream);

/* tap_decoder_step_hm with the same two masks at the same place (tap_decoder_step_dropout has the definition); the encoder
 * stage is untouched.  Launch record key (30, C, Np, Hd / 64, H, 2, 0). */
int tap_decoder_step_hm_dropout(tap_ctx *ctx, const float *xs, int Ks, const float *hm, int C, int W, int L, const float *h,
                                int B, int Hd, int m, const float *w1, const float *b1, const float *w2, const float *b2,
                                const float *w3, const float *b3, const float *P, const float *c, const float *w_hh,
                                const float *b_hh, const float *wq, const int64_t *state, uint32_t step, uint32_t env_offset,
                                uint32_t thr_rnn, uint32_t thr_hh, float s_rnn, float s_hh, float *h_out, float *q_out,
                                float *gates_out, float *enc_out, float *rnn_out, int64_t *keep_out, void *stream);

/* tap_decoder_step_backward for a step that ran with dropout, one element-wise launch, no atomics.  last_hh and rnn_out
 * both hang on h', so with g_h (B, Hd) the gradient at the returned last_hh, g_r (B, Hd) = g_q . wq (the caller's matmul)
 * and keep (B, 2, Hd / 64) as the forward wrote it:
 *   g = keep_hh s_hh g_h + keep_rnn s_rnn g_r        (each product and the sum rounded; a dropped element adds +0.0f)
 * and then tap_decoder_step_backward's formulas and outputs from g.  Checks as there; g_r and keep are required, keep
 * 8-byte aligned.  Launch record key (29, 0, TE, Hd / 64, H, 3, 0). */
int tap_decoder_step_dropout_backward(tap_ctx *ctx, int B, int Hd, const float *gates, const float *h, const float *g_h,
                                      const float *g_r, const int64_t *keep, float s_rnn, float s_hh, float *dgi_out,
                                      float *dghn_out, float *dh_carry_out, void *stream);

/* ---- the global pack-net's forward, one launch ------------------------------------------------ */
/* PackRNN.forward (pack_net/LG_RL.py:603-675) in its eval form for all B envs of a TAP_AT_NET descriptor: the encoder GRU
 * over the T columns of blocks (B, 2, T), then blocks_num decoder steps, each height-map input -> GRU cell -> fc ->
 * softmax -> first maximum -> PackEngine.step (tap_env_step_engine) -- the height-map never leaves the workgroup.
 * Notation: Hb = block_hidden_size, Hh = height_hidden_size, D = the decoder GRU's hidden size (Hb + Hh for G, 2 Hb + Hh for
 * LG), W' = W - 1 for the diff form, W otherwise.
 * Folds (the caller's, in torch, once per forward; they add no parameter):
 *   Pe (3 Hb, 2) = encoder.weight_ih_l0 . block_conv.weight      ce = encoder.bias_ih_l0 + encoder.weight_ih_l0 . block_conv.bias
 *   the columns of decoder.weight_ih_l0 are [encoder_last_hh (Hb) | block_vec (Hb, LG only) | height_vec (Hh)]:
 *   Pd_e (3 D, Hb) = the first Hb columns      Pd_b (3 D, 2; LG only) = block columns . block_conv.weight
 *   Pd_h (3 D, W') = height columns . height_map_conv.weight
 *   cd = bias_ih_l0 + height columns . height_map_conv.bias (+ block columns . block_conv.bias for LG)
 * Per env, fp32 throughout; every sum is ONE chain of fmaf in ascending term order, as in tap_decoder_step's contract;
 * sigmoid(x) = 1 / (1 + expf(-x)); the products r gh_n, (1 - z) n and z h are rounded before they are added.
 *   1. Encoder: h_e = 0; for t = 0 .. T - 1 (all T columns, not blocks_num; LG_RL.py:603-620): gi from ce over
 *      (blocks[b, 0, t], blocks[b, 1, t]), the raw floats; gh from enc_b_hh over the Hb terms of h_e (exactly enc_b_hh at
 *      t = 0); the GRU cell.  enc = h_e after T steps (dropout is the identity: the eval form only).
 *   2. u = the chain from cd over the Hb terms of enc with Pd_e: the constant part of the decoder's input, computed once
 *      and kept per env in the LDS.
 *   3. Decoder, i = 0 .. blocks_num - 1: x = the container's height-map in the form `form` -- full, zero (minus its
 *      minimum) or diff (hm[c + 1] - hm[c], W - 1 values); zeros at step 0 and after a wrap.  gi = the chain CONTINUED from
 *      u, for LG first over (blocks[b, 0, i], blocks[b, 1, i]) with Pd_b, then over x_0 .. x_{W' - 1} with Pd_h (the full
 *      chain's order); gh from dec_b_hh over the D terms of h_d (exactly dec_b_hh at i = 0); the cell gives h_d'.
 *      a = relu(chain from fc0_b over the D terms of h_d'); l_c = the chain from fc2_b[c] over the D terms of a, c < W;
 *      m = max l; column = the first c with l_c == m; s = sum_c exp((double)(l_c - m)), ascending, fp64;
 *      logp_out[b, i] = (float)(-log(s)).  Then the engine step at that column, tap_env_step_engine's rules exactly: clamp
 *      to W - w, z = max over the footprint, stability on the support row before the fill, empty = sum hm - valid, error
 *      bits 1 and 4, a start from empty at i % max_blocks == 0, the clear after (i + 1) % max_blocks == 0 (max_blocks == 0
 *      never wraps), the block is blocks[b, :, i] truncated, the tape is indexed by i, the 4th counter is i + 1, the error
 *      word restarts at step 0.  reward_out[b] = (C + P + S) / 3 in fp64, stored as f32, of the LAST step only, before a
 *      clear.
 * After the launch the state blob, tape, stability bytes and error words hold what blocks_num calls of tap_env_step_engine
 * with these columns leave, and reward_out what the last of them writes: every integer and the reward agree bit for bit.
 * feature_out (B, W') f32 or NULL: the next input.  No atomics, no cross-env sums: two calls give the same bytes, and an
 * env's bytes do not depend on the batch or the tile around it.  One launch, no allocation, no host read, no stream
 * synchronisation (capturable in a hipGraph).  k_pack_rnn_forward<KIND> (pack_rnn.hip): tap_decoder_step's geometry with
 * the loops over t and i inside the launch.  Launch record key (32, 2, TE, KIND, D / 64, 0, 0): TE = 16 envs per workgroup,
 * KIND a TAP_PACK_*.
 * Shapes: Hb = Hh = 128; kind G or LG; 2 <= W <= 64; the three forms; 1 <= blocks_num <= T <= the descriptor's tape;
 * max_blocks >= 0; anything else -> TAP_E_UNSUPPORTED.  Checks, in tap_decoder_step's order: a null descriptor or weights,
 * a descriptor that is not TAP_AT_NET, blocks_num outside [1, T] or max_blocks < 0 -> TAP_E_INVALID; B == 0 -> TAP_OK; a
 * null required buffer (Pd_b is required for LG only) or weights for another W -> TAP_E_INVALID; a shape outside the list
 * -> TAP_E_UNSUPPORTED; a state blob or a weight buffer that is not 16-byte aligned (the weight blocks are read 16 bytes at a
 * time), or another buffer that is not 4-byte aligned -> TAP_E_INVALID. */
enum { TAP_PACK_G = 0, TAP_PACK_LG = 1 };
typedef struct tap_pack_rnn_weights {
    int32_t kind;       /* TAP_PACK_* */
    int32_t Hb, Hh, W;
    int32_t form;       /* TAP_FEAT_*: the net's heightmap_type */
    int32_t reserved;
    const float *Pe, *ce, *enc_w_hh, *enc_b_hh;                 /* (3 Hb, 2), (3 Hb,), (3 Hb, Hb), (3 Hb,) */
    const float *Pd_e, *Pd_b, *Pd_h, *cd, *dec_w_hh, *dec_b_hh; /* (3 D, Hb), (3 D, 2) | NULL, (3 D, W'), (3 D,), (3 D, D), (3 D,) */
    const float *fc0_w, *fc0_b, *fc2_w, *fc2_b;                 /* (D, D), (D,), (W, D), (W,) */
} tap_pack_rnn_weights;
int tap_pack_rnn_forward(tap_ctx *ctx, const tap_env_desc *d, void *state, const float *blocks, int T, int blocks_num,
                         int max_blocks, const tap_pack_rnn_weights *w, float *logp_out, float *reward_out,
                         float *feature_out /* or NULL */, void *stream);

/* ---- the local pack-net's pick, one launch ---------------------------------------------------- */
/* tools.DQN.forward (tools.py:3322-3367) in its eval form, then the pick, for B envs: pnet + block -> the column, the log of
 * its probability and optionally the probabilities.  Notation: W columns, Wm = W - 1 map entries when the net drops the
 * map's last one (is_diff_height) else W, P = Wm + 2 positions along the conv axis (the map's entries, then the block's two
 * sides).
 * Folds (the caller's, in torch, once; tools.DQN.fold; they add no parameter), with s_i = bn_i.weight / sqrt(bn_i.running_var
 * + bn_i.eps):
 *   c1 (128, 4): per channel (a_m, b_m, a_b, b_b), a_m = s1 conv_height_map.weight, b_m = s1 (conv_height_map.bias - mean1)
 *      + bn1.bias, (a_b, b_b) the same from conv_block
 *   W2 (256, 128) = s2[:, None] conv2.weight, b2 = s2 (conv2.bias - mean2) + bn2.bias; W3 (256, 256), b3 likewise
 *   L1 (512, 256 P) = lin1.weight with its columns re-laid position-major (k = p 256 + c; the reference's flatten is c P + p)
 *   l1b = lin1.bias, head_w (W, 512), head_b (W,) unchanged
 * W2, W3 and L1 are handed over in the matrix cores' operand order, four steps of a lane together (T = 32, KS = 2 for W2 / W3;
 * T = 16, KS = 4 for L1; lane l < 64, i < 4):  Xp[q][tile][l][i] = X[tile T + l % T][KS (4 q + i) + l / T].
 * Per env b, fp32 unless said otherwise; every sum is ONE chain of fmaf in ascending term order from the bias (the f32-input
 * MFMA is bit for bit that chain):
 *   x_p = pnet[b pnet_stride + p] for p < Wm (the diff form's trailing entry is never read), block[b block_stride + p - Wm]
 *         for the last two positions
 *   h1[p][c] = max(0, fmaf(a[c], x_p, b[c])), the map's or the block's coefficients by position
 *   h2[p][o] = max(0, chain over c < 128 from b2[o]); h3[p][o] = max(0, chain over c < 256 of h2 from b3[o])
 *   y[o] = max(0, chain over k = p 256 + c from l1b[o]); l[c] = chain over the 512 terms of y from head_b[c]
 *   m = max l; x_out[b] = the first c with l_c == m; s = sum_c exp((double)(l_c - m)), ascending, fp64;
 *   logp_out[b] = (float)(-log(s)); probs_out[b, c] = (float)(exp((double)(l_c - m)) / s) when probs_out is given.
 * No split-K, no atomics, nothing crosses an env: two calls give the same bytes, and an env's bytes do not depend on B or on
 * its place in a tile.  One launch, no allocation, no host read, no stream synchronisation (capturable in a hipGraph).
 * k_dqn_pick<TE> (dqn.hip): a workgroup takes TE = 16 envs up to P = 7 and 8 up to P = 14; launch record key
 * (33, 2, TE, DIFF, P, 0, 0).  tap_dqn_pick_geometry (host only, no context) -> out[0] = TE, out[1] = P, out[2] = bytes of
 * dynamic LDS, or TAP_E_UNSUPPORTED.
 * Shapes: W >= 2 and P <= 14 (every W up to 12, and 13 in the diff form); anything else -> TAP_E_UNSUPPORTED.  Checks, in
 * tap_pack_rnn_forward's order: null weights, B < 0, or weights whose Wm is neither W nor W - 1 or whose P is not Wm + 2 ->
 * TAP_E_INVALID; B == 0 -> TAP_OK; a null required buffer, or an env stride below Wm / 2 floats -> TAP_E_INVALID; a shape
 * outside the list -> TAP_E_UNSUPPORTED; a weight buffer that is not 16-byte aligned, an x_out that is not 8-byte aligned or
 * another buffer that is not 4-byte aligned -> TAP_E_INVALID. */
typedef struct tap_dqn_weights {
    int32_t W, Wm, P, reserved;
    const float *c1;                    /* (128, 4) */
    const float *W2p, *b2, *W3p, *b3;   /* (16, 8, 64, 4), (256,), (32, 8, 64, 4), (256,) */
    const float *L1p, *l1b;             /* (16 P, 32, 64, 4), (512,) */
    const float *head_w, *head_b;       /* (W, 512), (W,) */
} tap_dqn_weights;
int tap_dqn_pick(tap_ctx *ctx, const tap_dqn_weights *w, const float *pnet, int pnet_stride, const float *block,
                 int block_stride, int B, int64_t *x_out, float *logp_out, float *probs_out /* or NULL */, void *stream);
int tap_dqn_pick_geometry(int W, int Wm, int32_t *out /* 3 ints, or NULL */);

/* ---- the step object of a decoding loop ----------------------------------------------------- */
/* DRL.forward's loop (model.py:342-496) runs its policy network between the environment steps, so the loop is
 * issued from the host, step by step, and what the host pays per step counts.  A tap_stepper is
 * tap_transition_first / tap_transition_bits with everything that does not change during an episode resolved
 * once: the caller allocates TWO phases of the step's outputs (the step of index k writes phase k & 1 and reads
 * phase (k & 1) ^ 1), the stepper remembers the pointers, alternates the phases, starts from a fresh container at
 * step 0 and emits calc_ratio at step `steps` - 1 -- one call with two arguments per step, no allocation, no
 * per-step argument marshalling.  The buffers stay the caller's (the library keeps no memory, only the addresses;
 * they must outlive the stepper).  Host-side object, not thread-safe; launches are asynchronous on `stream`. */
typedef struct tap_stepper tap_stepper;

typedef struct tap_stepper_buffers {
    unsigned long long *bits[2]; /* (B, nR) uint64 -- (B, 2, nR) above 64 rows: the bit shadow of dyn[w] */
    float *dyn[2];               /* (B, rows, nR): update_dynamic's result (pack.py:333-376) as the fp32 tensor model.py:378
                                    feeds the encoder.  Both NULL: the step keeps `dynamic` as bits[w] only and skips the
                                    expansion (78 % of a c2 step's bytes) -- for callers that consume the shadow; masks,
                                    placements, features and ratio are the same either way.
                                    dyn[0] == dyn[1] (windows with a bit shadow): ONE tensor, updated IN PLACE -- step 0 writes
                                    all of it, every later step only the rows it clears (pack.py:370-374: the result differs
                                    from the input in rows real + n*i alone; the reference's clone, pack.py:368, is there for
                                    autograd).  For loops under no_grad (validation, serving): the previous steps' tensors
                                    are gone.  The lane-per-cell fused steps (containers of at most 64 cells, MACS 2D up
                                    to 16 columns) write 3 rows per step instead of 3n; every other step form writes the whole
                                    tensor into the one buffer -- the same values either way */
    float *current[2];           /* (B, nR): update_mask's new_mask.float() (pack.py:329-331) */
    float *mask[2];              /* (B, nR): update_mask's chosen_mask */
    float *feature;              /* (B, feature_len) nullable: add_new_block's return, layout of model.py:456-465 */
    float *decoder_static;       /* (B, D) nullable: static[:, 1:1+D, ptr], the gather of model.py:404-406 */
    float *ratio;                /* (B,): calc_ratio, written by the last step (model.py:499-510) */
    int64_t *tour;               /* (B, tour_stride) nullable: column tour_col0 + k = the ptr of step k (model.py:495, 512) */
    int32_t *nonbinary;          /* device int32, nullable, caller zeroes it: see tap_mask_step_first */
    int32_t tour_stride;         /* 0 = steps */
    int32_t tour_col0;           /* first tour column this stepper writes (a rolling episode's last window: N - child) */
    float *colsum[2];            /* (B, 3, nR), only for windows WITHOUT a bit shadow (nR % 4 != 0, nR > 256 or rows > 128;
                                    NULL otherwise): the column-sum shadow of dyn[w]; the step is then tap_transition's
                                    fp32-copy form, dyn[] is required and bits[] is unused */
} tap_stepper_buffers;

/* d / state: the containers (tap_env_desc_init, a blob of tap_env_state_bytes); n, R, rows, update_rows,
 * static_rows as in tap_transition_bits; steps = decoding steps per episode (model.py:342: blocks_num).
 * Windows without a bit shadow (nR % 4 != 0, nR > 256, rows > 128) run tap_transition's fp32-copy form behind the same
 * three calls (buf->colsum; tap_stepper_begin then always makes its two small launches; tap_stepper_begin_shadow is
 * TAP_E_UNSUPPORTED there). */
int tap_stepper_create(tap_ctx *ctx, const tap_env_desc *d, void *state, int n, int R, int rows,
                       int update_rows, int static_rows, int steps, const tap_stepper_buffers *buf,
                       tap_stepper **out);
void tap_stepper_destroy(tap_stepper *s);

enum {
    TAP_SB_INITIAL_MASK = 1, /* tap_stepper_begin: also produce the masks DRL.forward starts from */
    TAP_SB_CONTINUE = 2      /* step 0 goes on with the containers as they are (rolling.py:428: one long-lived
                                container across the windows); default: step 0 starts from fresh containers */
};

/* Bind the next instance batch: static_ (B, static_rows, nR) and the fresh fp32 dynamic (B, rows, nR) a
 * DataLoader hands over (pack.py:195); both are only read and must stay valid for the episode.
 * TAP_SB_INITIAL_MASK: one launch builds the shadow and the masks DRL.forward starts from (model.py:297-307)
 * into phase 1 -- current[1] is what the policy sees before step 0.  Without it: no launch, step 0 reads the
 * tensor itself (a replayed tape needs no initial mask). */
int tap_stepper_begin(tap_stepper *s, const float *static_, const float *dyn_in, int flags, void *stream);

/* The same for a window whose bit shadow the caller already holds (tap_rolling_window / tap_rolling_step emit it
 * next to the tensor): step 0 reads `bits` (B, nR) -- not phase 0's buffer -- and starts from an all-ones mask.
 * No launch. */
int tap_stepper_begin_shadow(tap_stepper *s, const float *static_, const unsigned long long *bits, int flags);

/* One decoding step (model.py:376-465 in one launch, or the two launches tap_transition_bits runs for the shapes
 * without a single kernel): ptr (B,) int64.  Writes phase (k & 1) of bits / dyn / current / mask, plus feature,
 * decoder_static, tour[:, k] and -- at the last step -- ratio.  TAP_E_STEPS after `steps` steps. */
int tap_stepper_step(tap_stepper *s, const int64_t *ptr, void *stream);
/* steps taken since tap_stepper_begin */
int tap_stepper_steps_done(const tap_stepper *s);

/* The same for rolling.validate's loop (rolling.py:589-637; tap_rolling_window / tap_rolling_step): the caller
 * allocates two phases of the window's static tensor and node list (a step reads the current window's and writes
 * the next one's), one buffer of everything else; a step is one call with two arguments and its launch also
 * writes decoder_static, the tour column and the picked block's GLOBAL id (sub_graph_nodes[ptr], rolling.py:637).
 * After tap_roller_begin the first window is in phase 0; after step k the next window is in phase (k + 1) & 1.
 * After N - child steps the current window is the instance's last graph: run its episode with a tap_stepper
 * (tap_stepper_begin_shadow on static_[phase] and bits, TAP_SB_CONTINUE, tour_col0 = N - child). */
typedef struct tap_roller tap_roller;

typedef struct tap_roller_buffers {
    float *static_[2];              /* (B, 1+D, child*R) */
    int32_t *nodes[2];              /* (B, child): sorted global block ids = static's columns */
    float *dynamic;                 /* (B, 3*child, child*R); nullable when bits is given: no fp32 expansion */
    unsigned long long *bits;       /* (B, child*R) nullable: dynamic's bit shadow (needs 3*child <= 64) */
    float *colsum;                  /* (B, 3, child*R) nullable */
    float *current_mask;            /* (B, child*R) nullable (model.py:297-307) */
    int32_t *err;                   /* (B,) nullable: raised to 1 when a window could not be filled; cleared by begin */
    float *feature;                 /* (B, feature_len) nullable */
    float *decoder_static;          /* (B, D) nullable */
    int64_t *tour;                  /* (B, tour_stride) nullable: column k = the pick in window k */
    int32_t *picked;                /* (B, tour_stride) nullable: column k = global id of the block picked in window k */
    int32_t tour_stride;            /* >= N - child (N to leave room for the last window's episode) */
} tap_roller_buffers;

int tap_roller_create(tap_ctx *ctx, const tap_env_desc *d, void *env_state, int N, int child,
                      const tap_roller_buffers *buf, tap_roller **out);
void tap_roller_destroy(tap_roller *r);
/* blocks / rel / state as tap_rolling_init produced them (state is consumed: re-run tap_rolling_init, or restore
 * a saved copy, per episode).  Emits the first window into phase 0. */
int tap_roller_begin(tap_roller *r, const int32_t *blocks, const uint64_t *rel, uint64_t *state, void *stream);
/* place the block picked in the current window + emit the next window: tap_rolling_step */
int tap_roller_step(tap_roller *r, const int64_t *ptr, void *stream);
int tap_roller_steps_done(const tap_roller *r);

/* ---- the tail of a training iteration (train.hip) -------------------------------- */

/* trainer.py:216-225 in ONE launch.  reward (B,), critic_est (B,), tour_logp (B, n) float32 ->
 *   adv_out (B,)        reward - critic_est
 *   seed_logp_out (B, n) adv / B in every column: the gradient of mean(adv.detach() * tour_logp.sum(1))
 *   seed_est_out (B,)   -2 adv / B: the gradient of mean(adv^2) with respect to critic_est
 *   stats_out (5,)      actor_loss, critic_loss, mean reward, mean critic_est, number of flagged envs
 * An env whose reward is not finite (a flagged container under check='nan') has adv = 0 and zero seeds, is left out
 * of the four sums and is counted; the divisor stays B.  The sums are float64 in a fixed order (one thread per env,
 * 256 envs per workgroup, the workgroups' partials added in ascending order by the one that finishes last): the
 * same bytes on every call.  scratch: tap_reinforce_losses_scratch(B) bytes, 8-byte aligned, ZEROED by the caller
 * once and then left to the launches (its first word is their ticket).  B = 0 is TAP_OK and launches nothing. */
size_t tap_reinforce_losses_scratch(int B);
int tap_reinforce_losses(tap_ctx *ctx, const float *reward, const float *critic_est, const float *tour_logp, int B, int n,
                         float *adv_out, float *seed_logp_out, float *seed_est_out, float *stats_out, void *scratch,
                         size_t scratch_bytes, void *stream);

/* clip_grad_norm_ + Adam.step() for every parameter of several optimizers in two launches.  The caller cuts the
 * float32 parameters into chunks, one table entry each, the chunks of a group (one optimizer) contiguous: */
typedef struct tap_adam_chunk {
    float *param, *grad, *exp_avg, *exp_avg_sq; /* `count` elements each, 4-byte aligned; 16-byte accesses where all four are 16-byte aligned */
    int32_t count;                              /* >= 1 */
    int32_t group;
} tap_adam_chunk;
/* All arrays live on the device:
 *   ranges (groups, 2) int32    a group's first chunk and its number of chunks
 *   hyper (groups, 5) float64   lr, beta1, beta2, eps, max_norm -- read at every launch, so a new lr needs no re-capture
 *   steps (groups, 2) int64     the step counter, and the snapshot of it that tap_clip_adam_norm takes
 *   partials (chunks,) float64  tap_clip_adam_norm's output: the sum of squares of a chunk's gradient
 *   norms_out (groups,) float32 the gradient norm before clipping
 *   skipped (groups,) int32     goes up by one when a group's step was skipped
 * tap_clip_adam_apply adds a group's partials in ascending order, then coef = min(1, max_norm / (norm + 1e-6)) and
 * torch.optim.Adam's step (no weight decay, no amsgrad) on the clipped gradient, bias corrections from the counter,
 * which it advances; zero_grads != 0 zeroes the gradients.  A norm that is not finite skips that group: parameters,
 * moments and counter stay, the gradients are zeroed (zero_grads) and skipped goes up.  The two calls belong
 * together, in this order, on one stream.  chunks = 0 is TAP_OK and launches nothing. */
int tap_clip_adam_norm(tap_ctx *ctx, const tap_adam_chunk *table, int chunks, int groups, const int32_t *ranges,
                       int64_t *steps, double *partials, void *stream);
int tap_clip_adam_apply(tap_ctx *ctx, const tap_adam_chunk *table, int chunks, int groups, const int32_t *ranges,
                        const double *hyper, int64_t *steps, const double *partials, float *norms_out, int32_t *skipped,
                        int zero_grads, void *stream);

/* ---- measurement support ------------------------------------------------------------------ */

/* Bandwidth calibration in the hot kernels' own access shape (16 bytes per lane, a wavefront covers 1 KiB): SURVEY
 * 8(d) asks for the HBM peak to be confirmed on the box.  kind 0: dst = src (plain stores), 1: the same with
 * nontemporal stores, 2: fill dst (plain), 3: fill dst (nontemporal), 4: read src only, 5: fill with write-through
 * (sc0 sc1) stores, 6 / 7: the same in the bit-shadow expansion's store shape at c2 and as 4 800 linear bytes per wave
 * (bytes % 19200 == 0), 8: the same bytes as 960-byte store instructions that start on 64 bytes.  bytes % 16 == 0,
 * 16-byte aligned buffers.  scripts/calibrate_bw.py times these.  kinds 9 .. 13: SPARSE reads of src (256-byte aligned,
 * bytes % 256 == 0), one record per stride, every record once -- 9: 8 bytes of every 128, 10: 32 of 128, 11: 32 of 64,
 * 12: 64 of 128, 13: 32 of 256 -- for scripts/calibrate_fetch.py, which reads rocprofv3's FETCH_SIZE against them.
 * Nothing on the hot path calls these. */
int tap_bw_probe(tap_ctx *ctx, int kind, void *dst, const void *src, size_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TAPENV_H */
