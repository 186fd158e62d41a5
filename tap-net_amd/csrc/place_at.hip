// place_at.hip -- the learned local pack-net's environment step ("L-Pnet", reward types C+P+S-SL-soft / -RL-soft):
// a 2D block dropped at a column the CALLER chose, for B containers in lock-step.  Two seams of the reference with
// different rules (tapenv.h: tap_env_desc_set_place_at):
//   TAP_AT_CONTAINER  tools.Container.add_new_block_at (tools.py:3746-3822), what DRL_L's decoding loop calls
//                     (model.py:1211): stability is tested AFTER the cells under the block are filled, so it always
//                     holds; empty_size += the -1 cells under the block, old holes re-counted: sum_c (z - filled_c),
//                     filled_c = block cells of column c -- kept in the blob's per-column section
//   TAP_AT_NET        tools.calc_one_position_net (tools.py:3371-3461), what calc_positions_net / pack.reward /
//                     pack.render call: stability on the support row BEFORE the fill (a column carries the block iff
//                     its top is z, tools.is_stable_2d as in LB_GREEDY); empty_size = sum(heightmap) - valid_size
// Both: x = min(x, W - w) (the reference's `while x + w > W: x -= 1`), z = max(heightmap[x:x+w]), heightmap[x:x+w] =
// z + h.  A column x < 0 or a block wider than the container raises error bit 4 and is not placed; z + h > H raises
// bit 1 (the reference clips its numpy slices silently) and is placed, as LB_GREEDY does.
//
// Mapping: one lane per column, G = 8/16/32/64 lanes per container (tap_group_size), so several W = 5 containers share
// a wavefront; z, the support mask and the counter sums are group reductions (tap_place.h).  One launch per step also
// writes the decoder feature (the layout tap_env_step writes) and, optionally, the pack-net's input for the NEXT step.
//
// Engine mode (ENG, TAP_AT_NET only; tap_env_step_engine): the global pack-net's own environment, pack_net/LG_RL.py's
// PackEngine.step (LG_RL.py:440-496) at inner step `step` of a PackRNN forward.  Its placement, stability and
// empty_size are TAP_AT_NET's (on a height-map state LG_RL.is_stable_2d reads no -1 cell, so it agrees with
// tools.is_stable_2d).  What differs: the block is column `step` of blocks (B, 2, T) f32, read in place; a step with
// step % max_blocks == 0 starts from the empty container without reading the blob (the forward's clear, LG_RL.py:610-614,
// and the engine's wrap); the tape is written at index `step` and the 4th counter holds its length (step + 1, which
// tap_env_export reads as the steps taken); the reward (C+P+S)/3 is computed in fp64 and stored as
// f32 (LG_RL.py:460-475, 670); after the step that makes time == max_blocks the engine clears (LG_RL.py:482-491), so
// the blob and the next input are left empty -- the reward and the tape keep the values from before the clear.
// max_blocks = 0: never wraps, only step 0 starts empty (LG_RL.calc_positions' replay, LG_RL.py:714-727).
#include "tap_common.h"
#include "tap_place.h"

namespace {

struct AtArgs {
    tap_env_desc d;
    EnvView v;
    int32_t *col;          // [B][W] block cells per column (TAP_AT_CONTAINER)
    const void *blocks;    // (B, 2) f32 | i32, or null when gathering
    int blocks_dtype;
    const float *static_;  // gather source (B, static_rows, nR)
    int static_rows, nR;
    const int64_t *ptr;
    const int64_t *pos_x;  // (B,)
    const uint8_t *active;
    float *feature_out;
    int flen;
    float *pnet_out;       // (B, 1, W) or null
    int pnet_form;         // TAP_FEAT_*: full / zero / diff in DRL_L's form (length W, trailing 0)
    // engine mode (ENG): blocks is (B, 2, T) f32, column `step`; wrap period max_blocks (0 = never)
    int T, step, max_blocks;
    float *reward_out;     // (B,) f32 or null
};

template <int G, bool NET, bool ENG>
__global__ void __launch_bounds__(TAP_BLOCK) k_place_at(AtArgs a)
{
    static_assert(NET || !ENG, "the engine mode has TAP_AT_NET's rules");
    __shared__ int s_hm[TAP_BLOCK];
    const int tid = threadIdx.x, c = tid % G, lane = tid & 63, gl0 = lane - c;
    const int env = blockIdx.x * (TAP_BLOCK / G) + tid / G;
    const int W = a.d.W, B = a.d.B;
    const bool ev = env < B, incol = c < W;
    const int envc = ev ? env : 0;
    const int cc = min(c, W - 1);
    // loads first, unconditional on clamped addresses
    const long xraw = (long)a.pos_x[envc];
    long praw = 0;
    if (a.static_) praw = (long)a.ptr[envc];
    // engine mode: `start` = the container is empty before this step (nothing read), `wrap` = it is cleared after it
    const bool start = ENG && (a.max_blocks > 0 ? a.step % a.max_blocks == 0 : a.step == 0);
    const bool wrap = ENG && a.max_blocks > 0 && (a.step + 1) % a.max_blocks == 0;
    const int hm_l = start ? 0 : a.v.hm[(size_t)envc * W + cc];
    const int col_l = NET ? 0 : a.col[(size_t)envc * W + cc];
    const int4 cnt = start ? make_int4(0, 0, 0, 0) : reinterpret_cast<const int4 *>(a.v.cnt)[envc];
    unsigned char act_l = 1;
    if (a.active) act_l = a.active[envc];
    int bw, bh;
    if (a.static_) { // block = static[b, 1:3, ptr[b]] (model.py:404-412)
        bool badp;
        const long p = tap_col(praw, a.nR, badp);
        const float fw = a.static_[((size_t)envc * a.static_rows + 1) * a.nR + p];
        const float fh = a.static_[((size_t)envc * a.static_rows + 2) * a.nR + p];
        bw = badp ? 0 : (int)fw;
        bh = badp ? 0 : (int)fh;
    } else if (ENG) { // blocks[b, :, step], block.int() (LG_RL.py:450)
        const float *bp = (const float *)a.blocks + (size_t)envc * 2 * a.T + a.step;
        bw = (int)bp[0];
        bh = (int)bp[a.T];
    } else if (a.blocks_dtype == TAP_DT_F32) { // block.astype('int'), tools.py:3760
        bw = (int)((const float *)a.blocks)[(size_t)envc * 2];
        bh = (int)((const float *)a.blocks)[(size_t)envc * 2 + 1];
    } else {
        bw = ((const int32_t *)a.blocks)[(size_t)envc * 2];
        bh = ((const int32_t *)a.blocks)[(size_t)envc * 2 + 1];
    }
    const bool act = ev && act_l != 0;
    int err = 0;
    bool do_step = act;
    if (act && cnt.w >= a.d.n_max) { err |= 2; do_step = false; }          // tools.py:3677 IndexError
    if (act && (bw < 1 || bh < 1)) { err |= 4; do_step = false; }
    const long xl = min(xraw, (long)(W - bw));                             // tools.py:3765-3767
    if (do_step && xl < 0) { err |= 4; do_step = false; }                  // negative column / block wider than W
    const int x = do_step ? (int)xl : 0;
    const int w = do_step ? bw : 0;
    const bool inb = incol && c >= x && c < x + w;
    const int hm0 = incol ? hm_l : 0;
    const int z = group_max<G>(inb ? hm0 : 0);                             // tools.py:3770
    // support row: bit i = column x+i carries the block (its top is z); only the NET seam reads it
    const u64 wave_eq = __ballot(inb && hm0 == z);
    int hm = hm0, stab = 1, dcol = 0, col = col_l;
    if (do_step) {
        if (inb) {
            hm = z + bh;                                                   // tools.py:3786
            if (!NET) { dcol = z - col_l; col = col_l + bh; }              // the -1 cells under the block
        }
        if (NET && z > 0) {                                                // tools.py:3430-3434
            const u64 eq = (wave_eq >> (gl0 + x)) & (w >= 64 ? ~0ull : ((1ull << w) - 1ull));
            stab = tap_stable2d(w, eq);
        }
        if (z + bh > a.d.H) err |= 1;                                      // the reference clips silently
    }
    const int hsum = NET ? group_sum<G>(incol ? hm : 0) : 0;
    const int demp = NET ? 0 : group_sum<G>(dcol);
    const int hmax = ENG && a.reward_out ? group_max<G>(incol ? hm : 0) : 0;
    const int hm_w = wrap ? 0 : hm;                                        // what the blob and the next input see
    s_hm[tid] = hm_w;
    tap_wave_lds_sync();
    const int *s = s_hm + (tid - c);
    if (ev) {
        if (incol) {
            a.v.hm[(size_t)env * W + c] = hm_w;
            if (!NET && do_step && inb) a.col[(size_t)env * W + c] = col;
        }
        if (a.feature_out) tap_write_feature<2, G>(a.d.feature, W, 1, s, c, hm_w, a.feature_out + (size_t)env * a.flen);
        if (a.pnet_out) {                                                  // model.py:1173-1196 / tools.py:3407
            float *o = a.pnet_out + (size_t)env * W;
            if (a.pnet_form == TAP_FEAT_ZERO) {
                const int mn = group_min<G>(incol ? hm : INT_MAX);
                if (incol) o[c] = (float)(hm - mn);
            } else if (a.pnet_form == TAP_FEAT_DIFF) {
                if (incol) o[c] = (float)(c < W - 1 ? s[c + 1] - hm : 0);
            } else if (incol) {
                o[c] = (float)hm;
            }
        }
        if (c == 0) {
            const int4 now = do_step ? make_int4(cnt.x + bw * bh, 0, cnt.z + stab, cnt.w + 1) : cnt;
            const int valid = now.x;
            const int empty = !do_step ? cnt.y : NET ? hsum - valid : cnt.y + demp;
            // engine: the 4th counter is the forward's tape length (step + 1; tap_env_export shows that many rows), kept
            // across a wrap; the blocks since the last clear follow from the step (PackEngine counts every step)
            if (ENG)
                reinterpret_cast<int4 *>(a.v.cnt)[env] = wrap ? make_int4(0, 0, 0, a.step + 1)
                                                              : make_int4(valid, empty, now.z, a.step + 1);
            else if (do_step)
                reinterpret_cast<int4 *>(a.v.cnt)[env] = make_int4(valid, empty, now.z, now.w);
            if (do_step || ENG) {
                const int t = ENG ? a.step : cnt.w;                            // the engine's tape: by step index
                int32_t *q = a.v.pos + (size_t)t * 2 * B + env;
                q[0] = x;                                                      // (0, 0), unstable, for a refused step
                q[B] = z;
                a.v.stable[(size_t)t * B + env] = (uint8_t)(do_step ? stab : 0);
            }
            if (ENG && a.reward_out) {                                         // LG_RL.py:460-475, rw.astype('float32')
                const int since = (a.max_blocks > 0 ? a.step % a.max_blocks : a.step) + 1;
                const double box = (double)hmax * W, ve = (double)valid + (double)empty;
                const double C = box == 0 ? 0.0 : (double)valid / box;
                const double P = ve == 0 ? 0.0 : (double)valid / ve;
                const double S = (double)now.z / (double)since;
                a.reward_out[env] = (float)(((C + P) + S) / 3);
            }
            if (ENG && a.step == 0) a.v.err[env] = err;                        // errors of this forward only
            else if (err) a.v.err[env] |= err;
        }
    } else {
        // out-of-range groups take part in the group-wide reductions of the writers, so cross-lane ops stay convergent
        if (a.feature_out && a.d.feature == TAP_FEAT_ZERO) (void)group_min<G>(INT_MAX);
        if (a.pnet_out && a.pnet_form == TAP_FEAT_ZERO) (void)group_min<G>(INT_MAX);
    }
}

template <int G, bool NET, bool ENG> int launch_at(tap_ctx *ctx, const AtArgs &a, hipStream_t st)
{
    const int epb = TAP_BLOCK / G, grid = (a.d.B + epb - 1) / epb;
    hipLaunchKernelGGL((k_place_at<G, NET, ENG>), dim3(grid), dim3(TAP_BLOCK), 0, st, a);
    TAP_LAUNCH_CHECK(ctx, "k_place_at");
    tap_variant_hit(ctx, TAP_HIT_PLACE_AT, 2, G,
                    TapVariant{NET ? TAP_AT_NET : TAP_AT_CONTAINER, a.static_ ? 1 : 0, ENG ? 1 : 0}, 0);
    return TAP_OK;
}

template <bool NET, bool ENG = false> int dispatch_at(tap_ctx *ctx, int G, const AtArgs &a, hipStream_t st)
{
    if (G == 8) return launch_at<8, NET, ENG>(ctx, a, st);
    if (G == 16) return launch_at<16, NET, ENG>(ctx, a, st);
    if (G == 32) return launch_at<32, NET, ENG>(ctx, a, st);
    return launch_at<64, NET, ENG>(ctx, a, st);
}

int step_at_common(tap_ctx *ctx, const tap_env_desc *d, void *state, AtArgs &a, const int64_t *pos_x, float *pnet_out,
                   int pnet_form, void *stream)
{
    if (!d) return tap_fail(ctx, TAP_E_INVALID, "null descriptor");
    const int sem = tap_place_at_semantics(d);
    if (sem == 0) return tap_fail(ctx, TAP_E_INVALID, "step_at on a descriptor without place-at semantics (tap_env_desc_set_place_at)");
    if (sem < 0) return tap_fail(ctx, TAP_E_INVALID, "both place-at semantics set");
    if (d->D != 2) return tap_fail(ctx, TAP_E_INVALID, "place-at is 2D only (the reference's add_new_block_at unpacks two sides)");
    int rc = tap_desc_validate(ctx, d);
    if (rc) return rc;
    if (d->W > 64) return tap_fail(ctx, TAP_E_UNSUPPORTED, "place-at: W = %d columns > 64 lanes per container", d->W);
    if (pnet_out && pnet_form != TAP_FEAT_FULL && pnet_form != TAP_FEAT_ZERO && pnet_form != TAP_FEAT_DIFF)
        return tap_fail(ctx, TAP_E_INVALID, "bad pnet form %d", pnet_form);
    if (d->B == 0) return TAP_OK; // an empty batch has no buffers to check
    if (!state || !pos_x) return tap_fail(ctx, TAP_E_INVALID, "null state or pos_x");
    if (reinterpret_cast<uintptr_t>(state) % 16) return tap_fail(ctx, TAP_E_INVALID, "the state blob must be 16-byte aligned");
    a.d = *d;
    tap_env_layout(d, state, &a.v);
    a.col = reinterpret_cast<int32_t *>(static_cast<char *>(state) + tap_env_col_offset(d));
    a.pos_x = pos_x;
    a.pnet_out = pnet_out;
    a.pnet_form = pnet_form;
    a.flen = tap_env_feature_len(d);
    const int G = tap_group_size(d);
    if (a.T > 0) return dispatch_at<true, true>(ctx, G, a, (hipStream_t)stream);   // engine mode (checked TAP_AT_NET)
    return sem == TAP_AT_NET ? dispatch_at<true>(ctx, G, a, (hipStream_t)stream)
                             : dispatch_at<false>(ctx, G, a, (hipStream_t)stream);
}

} // namespace

extern "C" int tap_env_desc_set_place_at(tap_env_desc *d, int semantics)
{
    if (!d) return TAP_E_INVALID;
    if (semantics != 0 && semantics != TAP_AT_CONTAINER && semantics != TAP_AT_NET) return TAP_E_INVALID;
    if (semantics != 0 && d->D != 2) return TAP_E_INVALID;
    d->flags &= ~(TAP_F_AT_CONTAINER | TAP_F_AT_NET);
    if (semantics == TAP_AT_CONTAINER) d->flags |= TAP_F_AT_CONTAINER;
    if (semantics == TAP_AT_NET) d->flags |= TAP_F_AT_NET;
    return TAP_OK;
}

extern "C" int tap_env_step_at(tap_ctx *ctx, const tap_env_desc *d, void *state, const void *blocks, int blocks_dtype,
                               const uint8_t *active, float *feature_out, const int64_t *pos_x, float *pnet_out,
                               int pnet_form, void *stream)
{
    if (d && d->B == 0 && tap_place_at_semantics(d) > 0 && d->D == 2) return tap_desc_validate(ctx, d);
    if (d && d->B != 0 && !blocks) return tap_fail(ctx, TAP_E_INVALID, "null blocks");
    if (blocks_dtype != TAP_DT_F32 && blocks_dtype != TAP_DT_I32)
        return tap_fail(ctx, TAP_E_INVALID, "bad blocks_dtype %d", blocks_dtype);
    AtArgs a = {};
    a.blocks = blocks; a.blocks_dtype = blocks_dtype; a.active = active; a.feature_out = feature_out;
    return step_at_common(ctx, d, state, a, pos_x, pnet_out, pnet_form, stream);
}

extern "C" int tap_env_step_at_gather(tap_ctx *ctx, const tap_env_desc *d, void *state, const float *static_,
                                      int static_rows, int nR, const int64_t *ptr, const uint8_t *active,
                                      float *feature_out, const int64_t *pos_x, float *pnet_out, int pnet_form,
                                      void *stream)
{
    if (d && d->B == 0 && tap_place_at_semantics(d) > 0 && d->D == 2) return tap_desc_validate(ctx, d);
    if (!d || (d->B != 0 && (!static_ || !ptr || static_rows < 3 || nR < 1)))
        return tap_fail(ctx, TAP_E_INVALID, "bad gather arguments");
    AtArgs a = {};
    a.static_ = static_; a.static_rows = static_rows; a.nR = nR; a.ptr = ptr;
    a.active = active; a.feature_out = feature_out;
    return step_at_common(ctx, d, state, a, pos_x, pnet_out, pnet_form, stream);
}

extern "C" int tap_env_step_engine(tap_ctx *ctx, const tap_env_desc *d, void *state, const float *blocks, int T,
                                   int step, int max_blocks, const int64_t *pos_x, float *feature_out,
                                   float *reward_out, void *stream)
{
    if (!d) return tap_fail(ctx, TAP_E_INVALID, "null descriptor");
    if (tap_place_at_semantics(d) != TAP_AT_NET)
        return tap_fail(ctx, TAP_E_INVALID, "the engine step needs a TAP_AT_NET descriptor (tap_env_desc_set_place_at)");
    if (T < 1 || step < 0 || step >= T || max_blocks < 0)
        return tap_fail(ctx, TAP_E_INVALID, "engine step %d of T = %d columns, max_blocks %d", step, T, max_blocks);
    if (step >= d->n_max)
        return tap_fail(ctx, TAP_E_INVALID, "engine step %d beyond the descriptor's tape of %d", step, d->n_max);
    if (d->B == 0 && d->D == 2) return tap_desc_validate(ctx, d);
    if (d->B != 0 && !blocks) return tap_fail(ctx, TAP_E_INVALID, "null blocks");
    AtArgs a = {};
    a.blocks = blocks; a.blocks_dtype = TAP_DT_F32; a.feature_out = feature_out;
    a.T = T; a.step = step; a.max_blocks = max_blocks; a.reward_out = reward_out;
    return step_at_common(ctx, d, state, a, pos_x, nullptr, 0, stream);
}
