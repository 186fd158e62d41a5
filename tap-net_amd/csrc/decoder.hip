// decoder.hip -- the decoder side of a decoding step: the reference's decoder_static / decoder_dynamic encoders, their
// concatenation, the GRU cell of its pointer (one layer, one step) and the decoder's part of the attention, q (model.py:
// 347-354 and 108-115; tapenv.h: tap_decoder_step has the contract).  The encoders are 1x1 convolutions, so they fold into
// the GRU's input weights: gi = P . [xs ; xd] + c with K = Ks + Kd raw decoder values per env instead of Hd encoded ones.
// One launch goes from the stepper's two decoder buffers and last_hh to the new hidden state and q.
//
// Geometry.  Every product here is (a few hundred weight rows) x (a tile of envs), and the weights do not fit the LDS
// whole (W_hh is 196 KB at Hd = 128), so a workgroup takes DEC_TE = 4 DEC_E consecutive envs, keeps their h rows and
// their h' rows in the LDS for the whole launch, and streams the weights through the LDS in blocks of (64 hidden rows x
// their gates) x (DEC_KC = 32 terms): the hidden chunk is the OUTER loop, the term chunk the inner one, and the sums stay
// in registers across the term chunks.  A lane owns one hidden row j of the chunk and all three of its gates -- rows j,
// Hd + j, 2 Hd + j of the weights --, so the gate arithmetic needs no exchange; a wavefront owns DEC_E envs of the tile.
// Per four terms a lane reads one 16-byte piece per gate from the weight block (row stride DEC_WS = 36 floats: the 16
// lanes of a ds_read_b128 group fall on 16 different 4-bank slots) and one 16-byte piece per env from the activation
// tile (one address for the whole wavefront: a broadcast), and issues 12 DEC_E fused multiply-adds.  The input product
// runs the same code on a block of P and a (DEC_TE x DEC_KC) tile of [xs ; xd], zero-padded to a multiple of four terms;
// q runs it with one row per lane on Wq and the h' tile, after the barrier that completes h' of the tile.
//
// Every sum is ONE chain of fmaf in ascending term order: gi_g[j] from c[g Hd + j] over the K inputs (static columns
// first), gh_g[j] from b_hh[g Hd + j] over the Hd hidden terms, q[j] from 0 over the Hd terms of h'.  No atomics, no
// cross-lane sums, nothing depends on the batch or the tile: two calls give the same bytes, and an env's result does not
// depend on which other envs share its launch.
//
// Backward: element-wise only (k_decoder_step_bw), from the saved gates; the sums over the batch are the caller's GEMMs.
//
// Dropout form (training; tapenv.h: tap_decoder_step_dropout): the pointer's drop_hh and drop_rnn are two element-wise masks
// on h', applied where h' leaves the registers -- the value stored to h_out and the value written to the h' tile that q
// reads.  A lane draws its own (env, row) pair of keep bits from Philox4x32-10 (tap_decoder.h), keyed on a (seed, episode)
// pair read from device memory; a wavefront's 64 rows of an env are one ballot = one keep word.
//
// What is written here and what in tap_decoder.h.  The kernel is a template on its argument struct, and so are the pieces
// it shares with heightmap.hip's k_decoder_step_hm: the seed read, the h tile, the cell (dec_cell: gates, masks, keep
// words, stores) and q live once, in tap_decoder.h.  The two products that feed the cell stay written out in each kernel:
// the input product differs between the two, and moving the hidden product's block loop into a helper roughly doubles the
// packed multiply-adds and LDS reads of the gfx950 listing and takes the kernel from 152 to 242 VGPRs (DESIGN.md 7g has
// the figures).  The plain instantiation has no instruction of the dropout form: same registers, same count of every class
// of arithmetic and memory instruction as before the pieces moved.
#include "tap_decoder.h"

namespace {

constexpr int TAP_HIT_DECODER = 29;         // launch record (tapenv.h: tap_variant_hits), after pointer.hip's 28

struct DecArgs : DecCellArgs {
    const float *xs, *xd, *P;               // (B, Ks), (B, Kd), (3 Hd, K)
    int Ks, Kd;
};

inline size_t dec_lds_bytes(int Hd)
{
    return ((size_t)DEC_WROWS * DEC_WS + (size_t)DEC_TE * DEC_KC + 2 * (size_t)DEC_TE * Hd) * sizeof(float);   // 61 KB at Hd = 256
}

struct DecArgsDrop : DecArgs {
    DecDropArgs d;
};

// A = DecArgs: the plain step; A = DecArgsDrop: the dropout form (tapenv.h: tap_decoder_step_dropout), the two masks applied
// where h' leaves the registers -- nothing else of the launch differs, and the plain instantiation has no trace of it
template <typename A>
__global__ void __launch_bounds__(TAP_BLOCK) k_decoder_step(A a)
{
    extern __shared__ float4 dec_lds4[];                                   // (float4: the 16-byte reads need the base aligned)
    float *lw = reinterpret_cast<float *>(dec_lds4), *xa = lw + DEC_WROWS * DEC_WS, *hl = xa + DEC_TE * DEC_KC;
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX();
    const int B = a.B, Hd = a.Hd, Ks = a.Ks, K = a.Ks + a.Kd;
    float *hn = hl + DEC_TE * Hd;
    const int e0 = (int)blockIdx.x * DEC_TE, ew = wave * DEC_E;            // the tile's first env; the wavefront's first env in the tile
    const bool have_h = a.h != nullptr;
    const DecSeed seed = dec_seed(a);

    dec_load_h(a, hl, e0, tid);                                            // the first block's barriers publish the rows
    for (int jc = 0; jc < Hd / 64; ++jc) {
        const int j = jc * 64 + lane;
        float gi[3][DEC_E], gh[3][DEC_E];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const float ci = a.c[g * Hd + j], bi = a.b_hh[g * Hd + j];
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) { gi[g][e] = ci; gh[g][e] = bi; }
        }
        // gi += P . [xs ; xd]
        for (int k0 = 0; k0 < K; k0 += DEC_KC) {
            const int kn = min(DEC_KC, K - k0);
            __syncthreads();
            dec_fill_weights<3>(lw, a.P, K, Hd, jc * 64, k0, kn, tid);
#pragma unroll
            for (int it = 0; it < DEC_TE * DEC_KC / TAP_BLOCK; ++it) {
                const int i = it * TAP_BLOCK + tid, e = i / DEC_KC, kk = k0 + (i - e * DEC_KC), b = e0 + e;
                float v = 0.f;
                if (b < B && kk < K) v = kk < Ks ? a.xs[(size_t)b * Ks + kk] : a.xd[(size_t)b * a.Kd + (kk - Ks)];
                xa[i] = v;
            }
            __syncthreads();
            dec_mac<3>(lw, xa + ew * DEC_KC, DEC_KC, (kn + 3) >> 2, lane, gi);
        }
        // gh += W_hh . h (a null h is the zero state: gh stays b_hh).  Written out here and in k_decoder_step_hm, not a
        // helper of tap_decoder.h: see the opening comment
        if (have_h)
            for (int k0 = 0; k0 < Hd; k0 += DEC_KC) {
                __syncthreads();
                dec_fill_weights<3>(lw, a.w_hh, Hd, Hd, jc * 64, k0, DEC_KC, tid);
                __syncthreads();
                dec_mac<3>(lw, hl + ew * Hd + k0, Hd, DEC_KC / 4, lane, gh);
            }
        dec_cell(a, seed, gi, gh, hl, hn, e0, ew, jc, lane);
    }
    dec_q(a, lw, hn, e0, ew, lane, tid);
}

// the element-wise backward from the saved gates, and the same from a step that ran with dropout (tap_decoder.h: dec_step_bw)
__global__ void __launch_bounds__(TAP_BLOCK) k_decoder_step_bw(const float *gates, const float *h, const float *g_h, float *dgi, float *dghn,
                                                               float *carry, size_t total, int Hd)
{
    dec_step_bw<false>(gates, h, g_h, nullptr, nullptr, 0.f, 0.f, dgi, dghn, carry, total, Hd);
}

__global__ void __launch_bounds__(TAP_BLOCK) k_decoder_step_bw_drop(const float *gates, const float *h, const float *g_h, const float *g_r,
                                                                    const unsigned long long *keep, float s_rnn, float s_hh, float *dgi,
                                                                    float *dghn, float *carry, size_t total, int Hd)
{
    dec_step_bw<true>(gates, h, g_h, g_r, keep, s_rnn, s_hh, dgi, dghn, carry, total, Hd);
}

// What the dropout form of the backward takes beside the plain form's arguments
struct DecBwDrop {
    const float *g_r;                       // (B, Hd) g_q . wq
    const int64_t *keep;                    // the step's keep words
    float s_rnn, s_hh;
};

// the checks and the launch of both forms of the step: d null = the plain step; form = what its messages add to the name
int dec_step(tap_ctx *ctx, const DecArgs &a, const DecDropArgs *d, const char *form, void *stream)
{
    const int B = a.B, Hd = a.Hd, Ks = a.Ks, Kd = a.Kd;
    if (B < 0 || Ks < 0 || Kd < 0 || Hd < 1) return tap_fail(ctx, TAP_E_INVALID, "decoder step%s: B %d, Ks %d, Kd %d, Hd %d", form, B, Ks, Kd, Hd);
    if (B == 0) return TAP_OK; // an empty batch has no buffers to check
    if ((Ks > 0 && !a.xs) || (Kd > 0 && !a.xd) || !a.P || !a.c || !a.w_hh || !a.b_hh || !a.wq || !a.h_out || !a.q_out ||
        (d && dec_drop_null(d->state, d->keep)))
        return tap_fail(ctx, TAP_E_INVALID, "decoder step%s: null buffer", form);
    if (!dec_hd_ok(Hd) || Ks + Kd < 1 || Ks + Kd > Hd + 16)
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "decoder step%s: Ks %d, Kd %d, Hd %d (needs Hd 64, 128 or 256 and 1 <= Ks + Kd <= Hd + 16)", form, Ks,
                        Kd, Hd);
    const void *f32[] = {a.xs, a.xd, a.h, a.P, a.c, a.w_hh, a.b_hh, a.wq, a.h_out, a.q_out, a.gates_out, d ? d->rnn_out : nullptr};
    bool bad = d && dec_drop_misaligned(d->state, d->keep);
    for (const void *p : f32) bad = bad || dec_misaligned(p);
    if (bad)
        return tap_fail(ctx, TAP_E_INVALID, "decoder step%s: every %s", form,
                        d ? "float buffer must be 4-byte aligned, state and keep_out 8-byte" : "buffer must be 4-byte aligned");
    const dim3 blocks((unsigned)((B + DEC_TE - 1) / DEC_TE));
    if (d)
        hipLaunchKernelGGL(k_decoder_step<DecArgsDrop>, blocks, dim3(TAP_BLOCK), dec_lds_bytes(Hd), (hipStream_t)stream, DecArgsDrop{a, *d});
    else
        hipLaunchKernelGGL(k_decoder_step<DecArgs>, blocks, dim3(TAP_BLOCK), dec_lds_bytes(Hd), (hipStream_t)stream, a);
    TAP_LAUNCH_CHECK(ctx, d ? "k_decoder_step<dropout>" : "k_decoder_step");
    tap_variant_hit(ctx, TAP_HIT_DECODER, 0, DEC_TE, TapVariant{Hd / 64, a.h ? 1 : 0, d ? 2 : 0}, 0);
    return TAP_OK;
}

// the same for the element-wise backward
int dec_step_backward(tap_ctx *ctx, int B, int Hd, const float *gates, const float *h, const float *g_h, const DecBwDrop *d, float *dgi_out,
                      float *dghn_out, float *dh_carry_out, const char *form, void *stream)
{
    if (B < 0 || Hd < 1) return tap_fail(ctx, TAP_E_INVALID, "decoder step backward%s: B %d, Hd %d", form, B, Hd);
    if (B == 0) return TAP_OK; // (an empty batch leaves the outputs as they are)
    if (!gates || !g_h || (d && (!d->g_r || !d->keep)) || !dgi_out || !dghn_out || !dh_carry_out)
        return tap_fail(ctx, TAP_E_INVALID, "decoder step backward%s: null buffer", form);
    if (!dec_hd_ok(Hd)) return tap_fail(ctx, TAP_E_UNSUPPORTED, "decoder step backward%s: Hd %d (needs 64, 128 or 256)", form, Hd);
    const void *f32[] = {gates, h, g_h, d ? d->g_r : nullptr, dgi_out, dghn_out, dh_carry_out};
    bool bad = d && ((uintptr_t)d->keep & 7) != 0;
    for (const void *p : f32) bad = bad || dec_misaligned(p);
    if (bad)
        return tap_fail(ctx, TAP_E_INVALID, "decoder step backward%s: every %s", form,
                        d ? "float buffer must be 4-byte aligned, keep 8-byte" : "buffer must be 4-byte aligned");
    const size_t total = (size_t)B * Hd;
    const dim3 blocks((unsigned)((total + TAP_BLOCK - 1) / TAP_BLOCK));
    if (d)
        hipLaunchKernelGGL(k_decoder_step_bw_drop, blocks, dim3(TAP_BLOCK), 0, (hipStream_t)stream, gates, h, g_h, d->g_r,
                           (const unsigned long long *)d->keep, d->s_rnn, d->s_hh, dgi_out, dghn_out, dh_carry_out, total, Hd);
    else
        hipLaunchKernelGGL(k_decoder_step_bw, blocks, dim3(TAP_BLOCK), 0, (hipStream_t)stream, gates, h, g_h, dgi_out, dghn_out, dh_carry_out, total,
                           Hd);
    TAP_LAUNCH_CHECK(ctx, d ? "k_decoder_step_bw_drop" : "k_decoder_step_bw");
    tap_variant_hit(ctx, TAP_HIT_DECODER, 0, DEC_TE, TapVariant{Hd / 64, h ? 1 : 0, d ? 3 : 1}, 0);
    return TAP_OK;
}

} // namespace

extern "C" int tap_decoder_step_dropout(tap_ctx *ctx, const float *xs, int Ks, const float *xd, int Kd, const float *h, int B, int Hd,
                                        const float *P, const float *c, const float *w_hh, const float *b_hh, const float *wq,
                                        const int64_t *state, uint32_t step, uint32_t env_offset, uint32_t thr_rnn, uint32_t thr_hh,
                                        float s_rnn, float s_hh, float *h_out, float *q_out, float *gates_out, float *rnn_out,
                                        int64_t *keep_out, void *stream)
{
    const DecDropArgs d = {(const long long *)state, (unsigned long long *)keep_out, rnn_out, step, env_offset, thr_rnn, thr_hh, s_rnn, s_hh};
    return dec_step(ctx, {{h, c, w_hh, b_hh, wq, h_out, q_out, gates_out, B, Hd}, xs, xd, P, Ks, Kd}, &d, " (dropout)", stream);
}

extern "C" int tap_decoder_step_dropout_backward(tap_ctx *ctx, int B, int Hd, const float *gates, const float *h, const float *g_h,
                                                 const float *g_r, const int64_t *keep, float s_rnn, float s_hh, float *dgi_out,
                                                 float *dghn_out, float *dh_carry_out, void *stream)
{
    const DecBwDrop d = {g_r, keep, s_rnn, s_hh};
    return dec_step_backward(ctx, B, Hd, gates, h, g_h, &d, dgi_out, dghn_out, dh_carry_out, " (dropout)", stream);
}

extern "C" int tap_decoder_step(tap_ctx *ctx, const float *xs, int Ks, const float *xd, int Kd, const float *h, int B, int Hd,
                                const float *P, const float *c, const float *w_hh, const float *b_hh, const float *wq, float *h_out,
                                float *q_out, float *gates_out, void *stream)
{
    return dec_step(ctx, {{h, c, w_hh, b_hh, wq, h_out, q_out, gates_out, B, Hd}, xs, xd, P, Ks, Kd}, nullptr, "", stream);
}

extern "C" int tap_decoder_step_backward(tap_ctx *ctx, int B, int Hd, const float *gates, const float *h, const float *g_h, float *dgi_out,
                                         float *dghn_out, float *dh_carry_out, void *stream)
{
    return dec_step_backward(ctx, B, Hd, gates, h, g_h, nullptr, dgi_out, dghn_out, dh_carry_out, "", stream);
}
