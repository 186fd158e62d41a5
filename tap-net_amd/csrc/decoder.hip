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
// pair read from device memory; a wavefront's 64 rows of an env are one ballot = one keep word.  The kernel is a template on
// its argument struct: the plain instantiation's gfx950 listing is instruction for instruction what it was before the
// dropout form existed.
#include "tap_decoder.h"

namespace {

constexpr int TAP_HIT_DECODER = 29;         // launch record (tapenv.h: tap_variant_hits), after pointer.hip's 28

struct DecArgs {
    const float *xs, *xd, *h;               // (B, Ks), (B, Kd), (B, Hd) or null
    const float *P, *c, *w_hh, *b_hh, *wq;  // (3 Hd, K), (3 Hd,), (3 Hd, Hd), (3 Hd,), (Hd, Hd)
    float *h_out, *q_out, *gates_out;       // (B, Hd), (B, Hd), (B, 4, Hd) or null
    int B, Hd, Ks, Kd;
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
    constexpr bool DROP = std::is_same<A, DecArgsDrop>::value;
    extern __shared__ float4 dec_lds4[];                                   // (float4: the 16-byte reads need the base aligned)
    float *lw = reinterpret_cast<float *>(dec_lds4), *xa = lw + DEC_WROWS * DEC_WS, *hl = xa + DEC_TE * DEC_KC;
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX();
    const int B = a.B, Hd = a.Hd, Ks = a.Ks, K = a.Ks + a.Kd;
    float *hn = hl + DEC_TE * Hd;
    const int e0 = (int)blockIdx.x * DEC_TE, ew = wave * DEC_E;            // the tile's first env; the wavefront's first env in the tile
    const bool have_h = a.h != nullptr;
    unsigned seed_lo = 0, seed_hi = 0, episode = 0;
    if constexpr (DROP) {
        const unsigned long long seed = (unsigned long long)a.d.state[0];
        seed_lo = (unsigned)seed;
        seed_hi = (unsigned)(seed >> 32);
        episode = (unsigned)(unsigned long long)a.d.state[1];
    }

    // the tile's h rows (zeros for a null h and for the envs past the batch); the first block's barriers publish them
#pragma unroll 4
    for (int i = tid; i < DEC_TE * Hd; i += TAP_BLOCK) {
        const int e = i / Hd, k = i - e * Hd;
        hl[i] = (have_h && e0 + e < B) ? a.h[(size_t)(e0 + e) * Hd + k] : 0.f;
    }
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
        // gh += W_hh . h (a null h is the zero state: gh stays b_hh)
        if (have_h)
            for (int k0 = 0; k0 < Hd; k0 += DEC_KC) {
                __syncthreads();
                dec_fill_weights<3>(lw, a.w_hh, Hd, Hd, jc * 64, k0, DEC_KC, tid);
                __syncthreads();
                dec_mac<3>(lw, hl + ew * Hd + k0, Hd, DEC_KC / 4, lane, gh);
            }
#pragma unroll
        for (int e = 0; e < DEC_E; ++e) {
            const int b = e0 + ew + e;
            const float r = dec_sigmoid(gi[0][e] + gh[0][e]), z = dec_sigmoid(gi[1][e] + gh[1][e]);
            const float n = tanhf(gi[2][e] + r * gh[2][e]);
            const float hv = (1.f - z) * n + z * hl[(ew + e) * Hd + j];
            float h_rnn = hv, h_hh = hv;
            if constexpr (DROP) {
                bool keep_rnn, keep_hh;
                dec_keep(a.d, seed_lo, seed_hi, episode, b, j, keep_rnn, keep_hh);
                h_rnn = keep_rnn ? hv * a.d.s_rnn : 0.f;
                h_hh = keep_hh ? hv * a.d.s_hh : 0.f;
                const unsigned long long w_rnn = __ballot(keep_rnn), w_hh = __ballot(keep_hh);   // the wavefront's 64 rows of env b
                if (b < B) {
                    if (lane == 0) {
                        unsigned long long *kw = a.d.keep + (size_t)b * 2 * (Hd / 64) + jc;
                        kw[0] = w_rnn;
                        kw[Hd / 64] = w_hh;
                    }
                    if (a.d.rnn_out) a.d.rnn_out[(size_t)b * Hd + j] = h_rnn;
                }
            }
            hn[(ew + e) * Hd + j] = h_rnn;
            if (b < B) {
                a.h_out[(size_t)b * Hd + j] = h_hh;
                if (a.gates_out) {
                    float *go = a.gates_out + (size_t)b * 4 * Hd + j;
                    go[0] = r;
                    go[Hd] = z;
                    go[2 * Hd] = n;
                    go[3 * Hd] = gh[2][e];
                }
            }
        }
    }
    // q = Wq . h': the first block's barrier completes h' of the tile
    for (int jc = 0; jc < Hd / 64; ++jc) {
        const int j = jc * 64 + lane;
        float acc[1][DEC_E];
#pragma unroll
        for (int e = 0; e < DEC_E; ++e) acc[0][e] = 0.f;
        for (int k0 = 0; k0 < Hd; k0 += DEC_KC) {
            __syncthreads();
            dec_fill_weights<1>(lw, a.wq, Hd, 0, jc * 64, k0, DEC_KC, tid);
            __syncthreads();
            dec_mac<1>(lw, hn + ew * Hd + k0, Hd, DEC_KC / 4, lane, acc);
        }
#pragma unroll
        for (int e = 0; e < DEC_E; ++e)
            if (e0 + ew + e < B) a.q_out[(size_t)(e0 + ew + e) * Hd + j] = acc[0][e];
    }
}

// from h' = (1 - z) n + z h, n = tanh(gi_n + r gh_n), r / z = sigmoid(gi + gh): per element
//   carry = g z;  da_n = g (1 - z) (1 - n^2);  dgh_n = da_n r;  da_r = da_n gh_n r (1 - r);  da_z = g (h - n) z (1 - z)
__global__ void __launch_bounds__(TAP_BLOCK) k_decoder_step_bw(const float *gates, const float *h, const float *g_h, float *dgi, float *dghn,
                                                               float *carry, size_t total, int Hd)
{
    const size_t i = (size_t)blockIdx.x * TAP_BLOCK + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / (size_t)Hd;
    const int j = (int)(i - b * (size_t)Hd);
    const float *gp = gates + b * 4 * (size_t)Hd + j;
    const float r = gp[0], z = gp[Hd], n = gp[2 * Hd], ghn = gp[3 * Hd];
    const float g = g_h[i], hp = h ? h[i] : 0.f;
    const float dan = g * (1.f - z) * (1.f - n * n);
    float *dp = dgi + b * 3 * (size_t)Hd + j;
    dp[0] = dan * ghn * (r * (1.f - r));
    dp[Hd] = g * (hp - n) * (z * (1.f - z));
    dp[2 * Hd] = dan;
    dghn[i] = dan * r;
    carry[i] = g * z;
}

// the same from a step that ran with dropout: last_hh = drop_hh(h') and rnn_out = drop_rnn(h') both hang on h', so the
// gradient arriving at h' is g = keep_hh s_hh g_h + keep_rnn s_rnn g_r (g_r = g_q . wq, the caller's matmul), each product
// and the sum rounded; a dropped element contributes an exact zero
__global__ void __launch_bounds__(TAP_BLOCK) k_decoder_step_bw_drop(const float *gates, const float *h, const float *g_h, const float *g_r,
                                                                    const unsigned long long *keep, float s_rnn, float s_hh, float *dgi,
                                                                    float *dghn, float *carry, size_t total, int Hd)
{
    const size_t i = (size_t)blockIdx.x * TAP_BLOCK + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / (size_t)Hd;
    const int j = (int)(i - b * (size_t)Hd), nw = Hd >> 6;
    const unsigned long long *kw = keep + b * 2 * (size_t)nw + (j >> 6);
    const bool keep_rnn = (kw[0] >> (j & 63)) & 1, keep_hh = (kw[nw] >> (j & 63)) & 1;
    const float *gp = gates + b * 4 * (size_t)Hd + j;
    const float r = gp[0], z = gp[Hd], n = gp[2 * Hd], ghn = gp[3 * Hd];
    const float g = (keep_hh ? s_hh * g_h[i] : 0.f) + (keep_rnn ? s_rnn * g_r[i] : 0.f), hp = h ? h[i] : 0.f;
    const float dan = g * (1.f - z) * (1.f - n * n);
    float *dp = dgi + b * 3 * (size_t)Hd + j;
    dp[0] = dan * ghn * (r * (1.f - r));
    dp[Hd] = g * (hp - n) * (z * (1.f - z));
    dp[2 * Hd] = dan;
    dghn[i] = dan * r;
    carry[i] = g * z;
}

} // namespace

extern "C" int tap_decoder_step_dropout(tap_ctx *ctx, const float *xs, int Ks, const float *xd, int Kd, const float *h, int B, int Hd,
                                        const float *P, const float *c, const float *w_hh, const float *b_hh, const float *wq,
                                        const int64_t *state, uint32_t step, uint32_t env_offset, uint32_t thr_rnn, uint32_t thr_hh,
                                        float s_rnn, float s_hh, float *h_out, float *q_out, float *gates_out, float *rnn_out,
                                        int64_t *keep_out, void *stream)
{
    if (B < 0 || Ks < 0 || Kd < 0 || Hd < 1) return tap_fail(ctx, TAP_E_INVALID, "decoder step (dropout): B %d, Ks %d, Kd %d, Hd %d", B, Ks, Kd, Hd);
    if (B == 0) return TAP_OK; // an empty batch has no buffers to check
    if ((Ks > 0 && !xs) || (Kd > 0 && !xd) || !P || !c || !w_hh || !b_hh || !wq || !h_out || !q_out || dec_drop_null(state, keep_out))
        return tap_fail(ctx, TAP_E_INVALID, "decoder step (dropout): null buffer");
    if (!dec_hd_ok(Hd) || Ks + Kd < 1 || Ks + Kd > Hd + 16)
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "decoder step (dropout): Ks %d, Kd %d, Hd %d (needs Hd 64, 128 or 256 and 1 <= Ks + Kd <= Hd + 16)", Ks, Kd,
                        Hd);
    const void *f32[] = {xs, xd, h, P, c, w_hh, b_hh, wq, h_out, q_out, gates_out, rnn_out};
    bool bad = dec_drop_misaligned(state, keep_out);
    for (const void *p : f32) bad = bad || dec_misaligned(p);
    if (bad) return tap_fail(ctx, TAP_E_INVALID, "decoder step (dropout): every float buffer must be 4-byte aligned, state and keep_out 8-byte");
    const DecArgsDrop a = {{xs, xd, h, P, c, w_hh, b_hh, wq, h_out, q_out, gates_out, B, Hd, Ks, Kd},
                           {(const long long *)state, (unsigned long long *)keep_out, rnn_out, step, env_offset, thr_rnn, thr_hh, s_rnn, s_hh}};
    const unsigned blocks = (unsigned)((B + DEC_TE - 1) / DEC_TE);
    hipLaunchKernelGGL(k_decoder_step<DecArgsDrop>, dim3(blocks), dim3(TAP_BLOCK), dec_lds_bytes(Hd), (hipStream_t)stream, a);
    TAP_LAUNCH_CHECK(ctx, "k_decoder_step<dropout>");
    tap_variant_hit(ctx, TAP_HIT_DECODER, 0, DEC_TE, TapVariant{Hd / 64, h ? 1 : 0, 2}, 0);
    return TAP_OK;
}

extern "C" int tap_decoder_step_dropout_backward(tap_ctx *ctx, int B, int Hd, const float *gates, const float *h, const float *g_h,
                                                 const float *g_r, const int64_t *keep, float s_rnn, float s_hh, float *dgi_out,
                                                 float *dghn_out, float *dh_carry_out, void *stream)
{
    if (B < 0 || Hd < 1) return tap_fail(ctx, TAP_E_INVALID, "decoder step backward (dropout): B %d, Hd %d", B, Hd);
    if (B == 0) return TAP_OK; // (an empty batch leaves the outputs as they are)
    if (!gates || !g_h || !g_r || !keep || !dgi_out || !dghn_out || !dh_carry_out)
        return tap_fail(ctx, TAP_E_INVALID, "decoder step backward (dropout): null buffer");
    if (!dec_hd_ok(Hd)) return tap_fail(ctx, TAP_E_UNSUPPORTED, "decoder step backward (dropout): Hd %d (needs 64, 128 or 256)", Hd);
    const void *f32[] = {gates, h, g_h, g_r, dgi_out, dghn_out, dh_carry_out};
    bool bad = ((uintptr_t)keep & 7) != 0;
    for (const void *p : f32) bad = bad || dec_misaligned(p);
    if (bad) return tap_fail(ctx, TAP_E_INVALID, "decoder step backward (dropout): every float buffer must be 4-byte aligned, keep 8-byte");
    const size_t total = (size_t)B * Hd;
    hipLaunchKernelGGL(k_decoder_step_bw_drop, dim3((unsigned)((total + TAP_BLOCK - 1) / TAP_BLOCK)), dim3(TAP_BLOCK), 0, (hipStream_t)stream,
                       gates, h, g_h, g_r, (const unsigned long long *)keep, s_rnn, s_hh, dgi_out, dghn_out, dh_carry_out, total, Hd);
    TAP_LAUNCH_CHECK(ctx, "k_decoder_step_bw_drop");
    tap_variant_hit(ctx, TAP_HIT_DECODER, 0, DEC_TE, TapVariant{Hd / 64, h ? 1 : 0, 3}, 0);
    return TAP_OK;
}

extern "C" int tap_decoder_step(tap_ctx *ctx, const float *xs, int Ks, const float *xd, int Kd, const float *h, int B, int Hd,
                                const float *P, const float *c, const float *w_hh, const float *b_hh, const float *wq, float *h_out,
                                float *q_out, float *gates_out, void *stream)
{
    if (B < 0 || Ks < 0 || Kd < 0 || Hd < 1) return tap_fail(ctx, TAP_E_INVALID, "decoder step: B %d, Ks %d, Kd %d, Hd %d", B, Ks, Kd, Hd);
    if (B == 0) return TAP_OK; // an empty batch has no buffers to check
    if ((Ks > 0 && !xs) || (Kd > 0 && !xd) || !P || !c || !w_hh || !b_hh || !wq || !h_out || !q_out)
        return tap_fail(ctx, TAP_E_INVALID, "decoder step: null buffer");
    if (!dec_hd_ok(Hd) || Ks + Kd < 1 || Ks + Kd > Hd + 16)
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "decoder step: Ks %d, Kd %d, Hd %d (needs Hd 64, 128 or 256 and 1 <= Ks + Kd <= Hd + 16)", Ks, Kd, Hd);
    const void *f32[] = {xs, xd, h, P, c, w_hh, b_hh, wq, h_out, q_out, gates_out};
    bool bad = false;
    for (const void *p : f32) bad = bad || dec_misaligned(p);
    if (bad) return tap_fail(ctx, TAP_E_INVALID, "decoder step: every buffer must be 4-byte aligned");
    const DecArgs a = {xs, xd, h, P, c, w_hh, b_hh, wq, h_out, q_out, gates_out, B, Hd, Ks, Kd};
    const unsigned blocks = (unsigned)((B + DEC_TE - 1) / DEC_TE);
    hipLaunchKernelGGL(k_decoder_step<DecArgs>, dim3(blocks), dim3(TAP_BLOCK), dec_lds_bytes(Hd), (hipStream_t)stream, a);
    TAP_LAUNCH_CHECK(ctx, "k_decoder_step");
    tap_variant_hit(ctx, TAP_HIT_DECODER, 0, DEC_TE, TapVariant{Hd / 64, h ? 1 : 0, 0}, 0);
    return TAP_OK;
}

extern "C" int tap_decoder_step_backward(tap_ctx *ctx, int B, int Hd, const float *gates, const float *h, const float *g_h, float *dgi_out,
                                         float *dghn_out, float *dh_carry_out, void *stream)
{
    if (B < 0 || Hd < 1) return tap_fail(ctx, TAP_E_INVALID, "decoder step backward: B %d, Hd %d", B, Hd);
    if (B == 0) return TAP_OK; // (an empty batch leaves the outputs as they are)
    if (!gates || !g_h || !dgi_out || !dghn_out || !dh_carry_out) return tap_fail(ctx, TAP_E_INVALID, "decoder step backward: null buffer");
    if (!dec_hd_ok(Hd)) return tap_fail(ctx, TAP_E_UNSUPPORTED, "decoder step backward: Hd %d (needs 64, 128 or 256)", Hd);
    const void *f32[] = {gates, h, g_h, dgi_out, dghn_out, dh_carry_out};
    bool bad = false;
    for (const void *p : f32) bad = bad || dec_misaligned(p);
    if (bad) return tap_fail(ctx, TAP_E_INVALID, "decoder step backward: every buffer must be 4-byte aligned");
    const size_t total = (size_t)B * Hd;
    hipLaunchKernelGGL(k_decoder_step_bw, dim3((unsigned)((total + TAP_BLOCK - 1) / TAP_BLOCK)), dim3(TAP_BLOCK), 0, (hipStream_t)stream, gates, h,
                       g_h, dgi_out, dghn_out, dh_carry_out, total, Hd);
    TAP_LAUNCH_CHECK(ctx, "k_decoder_step_bw");
    tap_variant_hit(ctx, TAP_HIT_DECODER, 0, DEC_TE, TapVariant{Hd / 64, h ? 1 : 0, 1}, 0);
    return TAP_OK;
}
