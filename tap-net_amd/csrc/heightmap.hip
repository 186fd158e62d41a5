// heightmap.hip -- the decoder side of a 3D actor's decoding step: the reference's HeightmapEncoder (model.py:21-35: two
// strided 1x1 convolutions with leaky-ReLUs and a third whose kernel covers what is left of the map) in front of
// decoder.hip's step, in the same launch, workgroup and tile of envs (tapenv.h: tap_decoder_step_hm has the contract).
// The leaky-ReLUs keep the encoder from folding into the GRU's input weights, but it is small: both strides are 2 on
// kernel size 1, so only the cells (4i, 4j) of each plane are read -- Np = ceil(W / 4) ceil(L / 4) positions --, and the
// output is always 1 x 1: enc (m) per env, the dynamic half of decoder_hidden.
//
// Geometry: decoder.hip's (tap_decoder.h) -- a workgroup per DEC_TE = 16 consecutive envs, a wavefront per DEC_E = 4 of
// them, a lane per output row, weights through the LDS in 64 row x 32 term blocks.  The encoder stage runs first on the tile:
//   a1 (16 x Np x C1)   one thread per element, C <= 4 terms each, straight from the gathered cells in global memory;
//   a2 (16 x C2 Np)     w2 (C2, C1 <= 64) is at most two term blocks: both go into the weight region at once, one fill per
//                       64 rows, and the positions loop inside; stored as conv3.weight's memory order wants it, t = c2 Np + p;
//   enc (16 x m)        w3 (m, C2 Np) streams through in 32-term blocks, the sum in registers across them; a lane owns two
//                       rows (o, o + 64) where m >= 128, which halves the number of blocks and barriers.
// Then the step, as k_decoder_step runs it, except that the input product takes its dynamic terms from the enc tile in the
// LDS (the static columns are one block of their own, zero-padded to a multiple of four terms: fmaf(0, 0, s) = s).
// LDS: the weight block (27 KB) + the static tile (2 KB) + max(a1, enc) + max(a2, h and h' of the tile): a1 is dead when
// enc is written and a2 when h is loaded.  69 KB for the shipped actor (C 2, 5 x 5, m 128, Hd 256); 137 KB at the far
// corner of the supported list (m = Hd = 256, Np = 9).
//
// Every sum is ONE chain of fmaf in ascending term order, the encoder's three from their biases; no atomics, no
// cross-lane sums, nothing depends on the batch or the tile.  Backward: none here -- tap_decoder_step_backward from the
// saved gates, and the encoder's gradients are the caller's (rollout.decoder_step_heightmap recomputes a1 / a2 in torch).
// Dropout form (tapenv.h: tap_decoder_step_hm_dropout): decoder.hip's two masks at the same place, the encoder untouched;
// the kernel is a template on its argument struct, and the seed read, the h tile, the cell and q are tap_decoder.h's pieces,
// the same code k_decoder_step runs.  The two products in front of the cell are written out here (decoder.hip says why).
#include "tap_decoder.h"

namespace {

constexpr int TAP_HIT_HEIGHTMAP = 30;       // launch record (tapenv.h: tap_variant_hits), after decoder.hip's 29
constexpr int HM_MAX_SIDE = 12;             // W, L <= 12: Np <= 9

struct HmArgs : DecCellArgs {
    const float *xs, *hm;                   // (B, Ks), (B, C, W, L)
    const float *w1, *b1, *w2, *b2, *w3, *b3;   // (C1, C), (C1,), (C2, C1), (C2,), (m, C2 Np), (m,)
    const float *P;                         // (3 Hd, Ks + m)
    float *enc_out;                         // (B, m) or null
    int Ks, m, C, W, L, nl, Np;
};

inline size_t hm_r1_floats(int m, int Np) { return (size_t)DEC_TE * (size_t)std::max(Np * (m / 4), m); }
inline size_t hm_r2_floats(int m, int Np, int Hd) { return (size_t)DEC_TE * (size_t)std::max((m / 2) * Np, 2 * Hd); }
inline size_t hm_lds_bytes(int m, int Np, int Hd)
{
    return ((size_t)DEC_WROWS * DEC_WS + (size_t)DEC_TE * DEC_KC + hm_r1_floats(m, Np) + hm_r2_floats(m, Np, Hd)) * sizeof(float);
}

// dec_fill_weights for 64 NG consecutive rows of a matrix of `rows` rows, which need not be a multiple of 64: the rows
// past it are zeros.  A fill of its own: dec_fill_weights with the row bound as one more argument costs every step kernel
// 200 to 280 instructions and k_decoder_step three VGPRs
template <int NG>
__device__ __forceinline__ void hm_fill_rows(float *lw, const float *W, int ld, int rows, int row0, int k0, int kn, int tid)
{
    constexpr int N = NG * 64 * DEC_KC / TAP_BLOCK;
    float v[N];
#pragma unroll
    for (int it = 0; it < N; ++it) {
        const int i = it * TAP_BLOCK + tid, r = i / DEC_KC, k = i - r * DEC_KC;
        v[it] = (k < kn && row0 + r < rows) ? W[(unsigned)((row0 + r) * ld + k0 + k)] : 0.f;   // (w3 has at most 256 * 1152 elements)
    }
#pragma unroll
    for (int it = 0; it < N; ++it) {
        const int i = it * TAP_BLOCK + tid, r = i / DEC_KC, k = i - r * DEC_KC;
        lw[r * DEC_WS + k] = v[it];
    }
}

__device__ __forceinline__ float hm_leaky(float x) { return x > 0.f ? x : 0.01f * x; }

// enc[e][o] = b3[o] + sum_t w3[o][t] a2[e][t] for the tile, 64 NG rows per pass (a lane owns rows o, o + 64, ...): the
// first block's barrier completes a2; enc is written behind barriers that every wavefront's last read of a1 precedes
template <int NG>
__device__ __forceinline__ void hm_conv3(const HmArgs &a, float *lw, const float *a2, float *enc, int T, int e0, int ew, int lane, int tid)
{
    const int m = a.m;
    for (int oc = 0; oc * 64 * NG < m; ++oc) {
        float acc[NG][DEC_E];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int o = (oc * NG + g) * 64 + lane;
            const float bias = o < m ? a.b3[o] : 0.f;
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) acc[g][e] = bias;
        }
        for (int k0 = 0; k0 < T; k0 += DEC_KC) {
            const int kn = min(DEC_KC, T - k0);
            __syncthreads();
            hm_fill_rows<NG>(lw, a.w3, T, m, oc * 64 * NG, k0, kn, tid);
            __syncthreads();
            dec_mac<NG>(lw, a2 + ew * T + k0, T, kn >> 2, lane, acc);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int o = (oc * NG + g) * 64 + lane;
            if (o < m) {
#pragma unroll
                for (int e = 0; e < DEC_E; ++e) {
                    enc[(ew + e) * m + o] = acc[g][e];
                    if (a.enc_out && e0 + ew + e < a.B) a.enc_out[(size_t)(e0 + ew + e) * m + o] = acc[g][e];
                }
            }
        }
    }
}

struct HmArgsDrop : HmArgs {
    DecDropArgs d;
};

// A = HmArgs: the plain step; A = HmArgsDrop: the dropout form (tapenv.h: tap_decoder_step_hm_dropout), decoder.hip's two
// masks at the same place -- nothing else of the launch differs, and the plain instantiation has no trace of it
template <typename A>
__global__ void __launch_bounds__(TAP_BLOCK) k_decoder_step_hm(A a)
{
    extern __shared__ float4 hm_lds4[];                                   // (float4: the 16-byte reads need the base aligned)
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX();
    const int B = a.B, Hd = a.Hd, Ks = a.Ks, m = a.m, Np = a.Np, K = a.Ks + a.m;
    const int C1 = m >> 2, C2 = m >> 1, A1 = Np * C1, T = C2 * Np;         // a1 and a2 floats per env
    float *lw = reinterpret_cast<float *>(hm_lds4), *xa = lw + DEC_WROWS * DEC_WS, *r1 = xa + DEC_TE * DEC_KC;
    float *r2 = r1 + DEC_TE * max(A1, m);
    float *a1 = r1, *enc = r1, *a2 = r2, *hl = r2, *hn = r2 + DEC_TE * Hd;
    const int e0 = (int)blockIdx.x * DEC_TE, ew = wave * DEC_E;            // the tile's first env; the wavefront's first env in the tile
    const bool have_h = a.h != nullptr;
    const DecSeed seed = dec_seed(a);

    // ---- the encoder stage --------------------------------------------------------------------------------------------
    // a1[e][p][o] = leaky(b1[o] + sum_c w1[o][c] hm[b][c][4i][4j]), p = i nl + j (zeros for the envs past the batch)
    {
        const int C = a.C, plane = a.W * a.L;
        for (int i = tid; i < DEC_TE * A1; i += TAP_BLOCK) {
            const int e = i / A1, r = i - e * A1, p = r / C1, o = r - p * C1, b = e0 + e;
            float s = 0.f;
            if (b < B) {
                const int pi = p / a.nl, pj = p - pi * a.nl;
                const float *cell = a.hm + ((size_t)b * C * a.W + 4 * pi) * a.L + 4 * pj;
                s = a.b1[o];
                for (int cc = 0; cc < C; ++cc) s = fmaf(a.w1[o * C + cc], cell[cc * plane], s);
                s = hm_leaky(s);
            }
            a1[i] = s;
        }
    }
    // a2[e][o Np + p] = leaky(b2[o] + sum_c1 w2[o][c1] a1[e][p][c1]): the (at most two) term blocks of 64 rows of w2 side by side
    const int nkb = (C1 + DEC_KC - 1) / DEC_KC;
    for (int oc = 0; oc * 64 < C2; ++oc) {
        const int o = oc * 64 + lane;
        __syncthreads();                                                   // (a1 is complete; the previous rows' block has been consumed)
        for (int kb = 0; kb < nkb; ++kb)
            hm_fill_rows<1>(lw + kb * 64 * DEC_WS, a.w2, C1, C2, oc * 64, kb * DEC_KC, min(DEC_KC, C1 - kb * DEC_KC), tid);
        __syncthreads();
        const float bias = o < C2 ? a.b2[o] : 0.f;
        for (int p = 0; p < Np; ++p) {
            float acc[1][DEC_E];
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) acc[0][e] = bias;
            for (int kb = 0; kb < nkb; ++kb)
                dec_mac<1>(lw + kb * 64 * DEC_WS, a1 + ew * A1 + p * C1 + kb * DEC_KC, A1, min(DEC_KC, C1 - kb * DEC_KC) >> 2, lane, acc);
            if (o < C2) {
#pragma unroll
                for (int e = 0; e < DEC_E; ++e) a2[(ew + e) * T + o * Np + p] = hm_leaky(acc[0][e]);
            }
        }
    }
    // enc (it takes a1's place): two rows per lane where the encoder has them
    if (m >= 128)
        hm_conv3<2>(a, lw, a2, enc, T, e0, ew, lane, tid);
    else
        hm_conv3<1>(a, lw, a2, enc, T, e0, ew, lane, tid);
    __syncthreads();                                                      // a2 has been consumed: h and h' take its place

    // ---- the step, as k_decoder_step runs it --------------------------------------------------------------------------
    // the tile's h rows and its static values, zero-padded to a block; the first block's barriers publish them
    dec_load_h(a, hl, e0, tid);
#pragma unroll
    for (int it = 0; it < DEC_TE * DEC_KC / TAP_BLOCK; ++it) {
        const int i = it * TAP_BLOCK + tid, e = i / DEC_KC, kk = i - e * DEC_KC, b = e0 + e;
        xa[i] = (b < B && kk < Ks) ? a.xs[(size_t)b * Ks + kk] : 0.f;
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
        // gi += P . [xs ; enc]: the static columns, then the m dynamic ones from the enc tile
        if (Ks > 0) {
            __syncthreads();
            dec_fill_weights<3>(lw, a.P, K, Hd, jc * 64, 0, Ks, tid);
            __syncthreads();
            dec_mac<3>(lw, xa + ew * DEC_KC, DEC_KC, (Ks + 3) >> 2, lane, gi);
        }
        for (int d0 = 0; d0 < m; d0 += DEC_KC) {
            __syncthreads();
            dec_fill_weights<3>(lw, a.P, K, Hd, jc * 64, Ks + d0, DEC_KC, tid);
            __syncthreads();
            dec_mac<3>(lw, enc + ew * m + d0, m, DEC_KC / 4, lane, gi);
        }
        // gh += W_hh . h (a null h is the zero state: gh stays b_hh)
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

// the checks and the launch of both forms: d null = the plain step; form = what its messages add to "height-map"
int hm_step(tap_ctx *ctx, HmArgs a, const DecDropArgs *d, const char *form, void *stream)
{
    const int B = a.B, Hd = a.Hd, Ks = a.Ks, m = a.m, C = a.C, W = a.W, L = a.L;
    if (B < 0 || Ks < 0 || C < 1 || W < 1 || L < 1 || Hd < 1 || m < 1)
        return tap_fail(ctx, TAP_E_INVALID, "decoder step (height-map%s): B %d, Ks %d, C %d, W %d, L %d, Hd %d, m %d", form, B, Ks, C, W, L, Hd, m);
    if (B == 0) return TAP_OK; // an empty batch has no buffers to check
    if ((Ks > 0 && !a.xs) || !a.hm || !a.w1 || !a.b1 || !a.w2 || !a.b2 || !a.w3 || !a.b3 || !a.P || !a.c || !a.w_hh || !a.b_hh || !a.wq ||
        !a.h_out || !a.q_out || (d && dec_drop_null(d->state, d->keep)))
        return tap_fail(ctx, TAP_E_INVALID, "decoder step (height-map%s): null buffer", form);
    if (!dec_hd_ok(Hd) || (m != Hd && 2 * m != Hd) || (C != 1 && C != 2 && C != 4) || W > HM_MAX_SIDE || L > HM_MAX_SIDE || Ks > 16 ||
        Ks + m > Hd + 16)
        return tap_fail(ctx, TAP_E_UNSUPPORTED,
                        "decoder step (height-map%s): Ks %d, C %d, W %d, L %d, m %d, Hd %d (needs Hd 64, 128 or 256, m = Hd / 2 or Hd, C 1, 2 or 4, "
                        "W and L <= 12, Ks <= 16 and Ks + m <= Hd + 16)", form, Ks, C, W, L, m, Hd);
    const void *f32[] = {a.xs, a.hm, a.h, a.w1, a.b1, a.w2, a.b2, a.w3, a.b3, a.P, a.c, a.w_hh, a.b_hh, a.wq, a.h_out, a.q_out, a.gates_out,
                         a.enc_out, d ? d->rnn_out : nullptr};
    bool bad = d && dec_drop_misaligned(d->state, d->keep);
    for (const void *p : f32) bad = bad || dec_misaligned(p);
    if (bad)
        return tap_fail(ctx, TAP_E_INVALID, "decoder step (height-map%s): every %s", form,
                        d ? "float buffer must be 4-byte aligned, state and keep_out 8-byte" : "buffer must be 4-byte aligned");
    a.nl = (L + 3) / 4;
    a.Np = ((W + 3) / 4) * a.nl;
    const size_t lds = hm_lds_bytes(m, a.Np, Hd);
    if (lds > tap_lds_limit(ctx))
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "decoder step (height-map%s): %zu bytes of LDS for m %d, Np %d, Hd %d do not fit a workgroup", form,
                        lds, m, a.Np, Hd);
    const dim3 blocks((unsigned)((B + DEC_TE - 1) / DEC_TE));
    if (d) {
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_decoder_step_hm<HmArgsDrop>, lds));
        hipLaunchKernelGGL(k_decoder_step_hm<HmArgsDrop>, blocks, dim3(TAP_BLOCK), lds, (hipStream_t)stream, HmArgsDrop{a, *d});
    } else {
        TAP_HIP_CHECK(ctx, tap_allow_lds(k_decoder_step_hm<HmArgs>, lds));
        hipLaunchKernelGGL(k_decoder_step_hm<HmArgs>, blocks, dim3(TAP_BLOCK), lds, (hipStream_t)stream, a);
    }
    TAP_LAUNCH_CHECK(ctx, d ? "k_decoder_step_hm<dropout>" : "k_decoder_step_hm");
    tap_variant_hit(ctx, TAP_HIT_HEIGHTMAP, C, a.Np, TapVariant{Hd / 64, a.h ? 1 : 0, d ? 2 : 0}, 0);
    return TAP_OK;
}

} // namespace

extern "C" int tap_decoder_step_hm(tap_ctx *ctx, const float *xs, int Ks, const float *hm, int C, int W, int L, const float *h, int B, int Hd,
                                   int m, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                                   const float *b3, const float *P, const float *c, const float *w_hh, const float *b_hh, const float *wq,
                                   float *h_out, float *q_out, float *gates_out, float *enc_out, void *stream)
{
    return hm_step(ctx, {{h, c, w_hh, b_hh, wq, h_out, q_out, gates_out, B, Hd}, xs, hm, w1, b1, w2, b2, w3, b3, P, enc_out, Ks, m, C, W, L, 0, 0},
                   nullptr, "", stream);
}

extern "C" int tap_decoder_step_hm_dropout(tap_ctx *ctx, const float *xs, int Ks, const float *hm, int C, int W, int L, const float *h, int B,
                                           int Hd, int m, const float *w1, const float *b1, const float *w2, const float *b2,
                                           const float *w3, const float *b3, const float *P, const float *c, const float *w_hh,
                                           const float *b_hh, const float *wq, const int64_t *state, uint32_t step, uint32_t env_offset,
                                           uint32_t thr_rnn, uint32_t thr_hh, float s_rnn, float s_hh, float *h_out, float *q_out,
                                           float *gates_out, float *enc_out, float *rnn_out, int64_t *keep_out, void *stream)
{
    const DecDropArgs d = {(const long long *)state, (unsigned long long *)keep_out, rnn_out, step, env_offset, thr_rnn, thr_hh, s_rnn, s_hh};
    return hm_step(ctx, {{h, c, w_hh, b_hh, wq, h_out, q_out, gates_out, B, Hd}, xs, hm, w1, b1, w2, b2, w3, b3, P, enc_out, Ks, m, C, W, L, 0, 0},
                   &d, ", dropout", stream);
}
