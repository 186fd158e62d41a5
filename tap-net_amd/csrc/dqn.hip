// dqn.hip -- the local pack-net's eval forward in ONE launch (tools.DQN, tools.py:3322-3367; tapenv.h: tap_dqn_pick has the
// contract): layer 1 -> conv2 -> conv3 -> lin1 -> head -> softmax -> first maximum, for all B envs, from the folded weights
// of tools.DQN.fold().  The three GEMMs run on the f32-input matrix cores (v_mfma_f32_32x32x2_f32 for conv2 / conv3,
// v_mfma_f32_16x16x4_f32 for lin1), whose result is bit for bit a k-ordered fmaf chain from the accumulator's initial value
// -- the bias --, so every sum is ONE chain in ascending term order, as in every other launch of this library.
//
// Geometry: a workgroup of four wavefronts takes TE consecutive envs (16 up to P = 7 positions, 8 up to P = 14), i.e.
// R = TE P rows of the position-wise layers, in blocks of 32 rows:
//   conv2  M = 32 rows, N = 256 (a wavefront 64 columns = two 32 x 32 tiles), K = 128.  The A operand is never stored: a
//          lane computes h1[row][c] = max(0, fmaf(a[c], x_row, b[c])) from its row's scalar input as the MFMA needs it.
//          The result, relu'd, goes to the LDS tile h2 (32 x 256) in conv3's operand order.
//   conv3  the same with K = 256 from the h2 tile; the result goes to the resident LDS tile h3 (R x 256) in lin1's order.
//   lin1   M = 16 envs (rows past TE repeat the last env and are dropped), N = 512 (a wavefront 128 columns = eight
//          16 x 16 tiles), K = 256 P over the h3 tile, k = p 256 + c.  The result, relu'd, goes to y (TE x 512), in the dead
//          h2 tile.
//   head   a lane per (env, column): the chain over y's 512 terms; then a lane per env: maximum, first maximum, the fp64
//          softmax terms in ascending order (tap_pack_rnn_forward's head).
// Operand order.  An MFMA step consumes KS = 2 (32x32x2) or 4 (16x16x4) terms, lane l holding term k = KS kk + l / T of row /
// column l % T (T = 32 | 16).  A lane's terms of four consecutive steps are stored together, so one 16-byte load feeds four
// MFMAs: the weights come packed that way from fold() (Wp[q][tile][lane][i] = W[tile T + l % T][KS (4 q + i) + l / T]) and
// stream from L2 straight into the B operand, one step quad ahead of the multiplies; the activation tiles keep row r as
// [l / T][kk] (element [g][kk] = channel KS kk + g), rows DQN_RS = 260 floats apart.
//
// LDS, floats: h3 TE P x 260 | h2 32 x 260 (later y, TE x 516) | layer-1 coefficients 128 x 4 | logits TE x 16: 135 KB at
// TE = 16, P = 6 -- one workgroup per CU, one wavefront per SIMD.  DESIGN.md 7q has the figures.
//
// Nothing crosses an env, there is no split-K and no atomic: two calls give the same bytes, and an env's bytes do not depend
// on the batch or on its place in a tile (an MFMA's output element depends on its own row and column only).
#include "tap_common.h"

namespace {

constexpr int TAP_HIT_DQN = 33;             // launch record (tapenv.h: tap_variant_hits), after pack_rnn.hip's 32
constexpr int DQN_C1 = 128, DQN_C2 = 256, DQN_H = 512;   // the reference's channel counts (tools.py:3325-3338)
constexpr int DQN_RS = DQN_C2 + 4;          // row stride of the h2 / h3 tiles, floats
constexpr int DQN_YS = DQN_H + 4;           // row stride of y
constexpr int DQN_LS = 16;                  // row stride of the logits: W <= 13
constexpr int DQN_PMAX = 14;                // positions: 8 envs x 14 rows is what the LDS holds

typedef float dqn_f16 __attribute__((ext_vector_type(16)));
typedef float dqn_f4 __attribute__((ext_vector_type(4)));

struct DqnArgs {
    tap_dqn_weights w;
    const float *pnet, *block;
    int pnet_stride, block_stride, B;
    int64_t *x;
    float *logp, *probs;
};

inline int dqn_te(int P) { return P <= 7 ? 16 : 8; }
inline size_t dqn_lds_bytes(int TE, int P)
{
    return ((size_t)TE * P * DQN_RS + 32 * DQN_RS + 4 * DQN_C1 + (size_t)TE * DQN_LS) * sizeof(float);
}

__device__ __forceinline__ float dqn_el(const float4 &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// one 32-row block of conv2 or conv3 for this wavefront's 64 output columns: acc = bias, K / 8 step quads, two tiles.
// LAYER1: the A operand is layer 1, computed from the lane's input x (sel: the block's coefficients); otherwise it is read from
// the h2 tile.  Wp: the packed weights, bias (256).  The relu'd result goes to `out` (rows row0 .. of stride DQN_RS, rows >=
// nrows dropped) in the operand order of a consumer with KS_OUT terms per step.
template <bool LAYER1, int K, int KS_OUT>
__device__ __forceinline__ void dqn_conv(const float *Wp, const float *bias, const float *coef, float x, bool sel, const float *hin,
                                         float *out, int nrows, int wave, int lane)
{
    const int j = lane & 31, h = lane >> 5;
    dqn_f16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float b = bias[(2 * wave + t) * 32 + j];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = b;
    }
    const float4 *wp = reinterpret_cast<const float4 *>(Wp) + (size_t)(2 * wave) * 64 + lane;   // [q][tile][lane]
    constexpr int NT = DQN_C2 / 32, Q = K / 8;
    float4 bn[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) bn[t] = wp[t * 64];
    for (int q = 0; q < Q; ++q) {
        float4 bc[2] = {bn[0], bn[1]};
        if (q + 1 < Q) {
#pragma unroll
            for (int t = 0; t < 2; ++t) bn[t] = wp[(size_t)(q + 1) * NT * 64 + t * 64];
        }
        float4 a4;
        if constexpr (!LAYER1) a4 = *reinterpret_cast<const float4 *>(hin + j * DQN_RS + h * (K / 2) + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float a;
            if constexpr (LAYER1) {
                const float4 c = *reinterpret_cast<const float4 *>(coef + 4 * (2 * (4 * q + i) + h));   // a_m, b_m, a_b, b_b
                a = fmaxf(0.f, fmaf(sel ? c.z : c.x, x, sel ? c.w : c.y));
            } else {
                a = dqn_el(a4, i);
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dqn_el(bc[t], i), acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int o = (2 * wave + t) * 32 + j;                                 // the output channel: the consumer's term
        const int off = (o % KS_OUT) * (DQN_C2 / KS_OUT) + o / KS_OUT;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row < nrows) out[row * DQN_RS + off] = fmaxf(0.f, acc[t][r]);
        }
    }
}

// The per-step body: TE envs from env e0 on.  Written so that a later whole-tour kernel can call it in a loop over the blocks.
template <int TE>
__device__ __forceinline__ void dqn_step(const DqnArgs &a, float *lds, int e0, int tid)
{
    const tap_dqn_weights &w = a.w;
    const int P = w.P, Wm = w.Wm, W = w.W, B = a.B, R = TE * P;
    const int lane = tid & 63, wave = TAP_WAVE_INDEX();
    float *h3 = lds, *h2 = h3 + TE * P * DQN_RS, *coef = h2 + 32 * DQN_RS, *logit = coef + 4 * DQN_C1, *y = h2;

    for (int i = tid; i < 4 * DQN_C1; i += TAP_BLOCK) coef[i] = w.c1[i];
    __syncthreads();

    // ---- the position-wise layers, 32 rows at a time -----------------------------------------------------------------
    for (int row0 = 0; row0 < R; row0 += 32) {
        const int row = row0 + (lane & 31);
        float x = 0.f;
        bool sel = false;
        if (row < R) {
            const int e = row / P, p = row - e * P;
            const size_t b = (size_t)min(e0 + e, B - 1);                       // an env past the batch reads the last one's
            sel = p >= Wm;
            x = sel ? a.block[b * a.block_stride + (p - Wm)] : a.pnet[b * a.pnet_stride + p];
        }
        dqn_conv<true, DQN_C1, 2>(w.W2p, w.b2, coef, x, sel, nullptr, h2, 32, wave, lane);
        __syncthreads();
        dqn_conv<false, DQN_C2, 4>(w.W3p, w.b3, nullptr, 0.f, false, h2, h3 + row0 * DQN_RS, R - row0, wave, lane);
        __syncthreads();                                                       // the h2 tile is free again; h3's rows are in
    }

    // ---- lin1: y = relu(L1 . h3 + b), k = p 256 + c ---------------------------------------------------------------------
    {
        const int j = lane & 15, g = lane >> 4, m = min(j, TE - 1);
        dqn_f4 acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float b = w.l1b[(8 * wave + t) * 16 + j];
            acc[t] = dqn_f4{b, b, b, b};
        }
        constexpr int NT = DQN_H / 16;
        const float4 *wp = reinterpret_cast<const float4 *>(w.L1p) + (size_t)(8 * wave) * 64 + lane;   // [q][tile][lane]
        const int Q = P * (DQN_C2 / 16);
        float4 bn[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) bn[t] = wp[t * 64];
        for (int q = 0; q < Q; ++q) {
            float4 bc[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) bc[t] = bn[t];
            if (q + 1 < Q) {
#pragma unroll
                for (int t = 0; t < 8; ++t) bn[t] = wp[(size_t)(q + 1) * NT * 64 + t * 64];
            }
            const int p = q >> 4, qq = q & 15;
            const float4 a4 = *reinterpret_cast<const float4 *>(h3 + (m * P + p) * DQN_RS + g * (DQN_C2 / 4) + 4 * qq);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float av = dqn_el(a4, i);
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, dqn_el(bc[t], i), acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int o = (8 * wave + t) * 16 + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 4 * g + r;
                if (e < TE) y[e * DQN_YS + o] = fmaxf(0.f, acc[t][r]);
            }
        }
    }
    __syncthreads();

    // ---- head: a lane per (env, column) ---------------------------------------------------------------------------------
    {
        const int e = 4 * wave + (lane >> 4), c = lane & 15;
        if (e < TE) {
            const int cc = min(c, W - 1);
            float l = w.head_b[cc];
            const float4 *hw = reinterpret_cast<const float4 *>(w.head_w + (size_t)cc * DQN_H);
            const float4 *yr = reinterpret_cast<const float4 *>(y + e * DQN_YS);
#pragma unroll 4
            for (int k4 = 0; k4 < DQN_H / 4; ++k4) {
                const float4 yv = yr[k4], wv = hw[k4];
                l = fmaf(wv.x, yv.x, l);
                l = fmaf(wv.y, yv.y, l);
                l = fmaf(wv.z, yv.z, l);
                l = fmaf(wv.w, yv.w, l);
            }
            logit[e * DQN_LS + c] = l;
        }
    }
    __syncthreads();
    // ---- the pick, a lane per env (tap_pack_rnn_forward's head) ------------------------------------------------------------
    if (tid < TE && e0 + tid < B) {
        const size_t b = (size_t)(e0 + tid);
        const float *l = logit + tid * DQN_LS;
        float m = l[0];
        int pick = 0;
        for (int c = 1; c < W; ++c)
            if (l[c] > m) { m = l[c]; pick = c; }                              // the first maximum
        double s = 0.0;
        for (int c = 0; c < W; ++c) s += exp((double)(l[c] - m));
        a.x[b] = pick;
        a.logp[b] = (float)(-log(s));
        if (a.probs)
            for (int c = 0; c < W; ++c) a.probs[b * W + c] = (float)(exp((double)(l[c] - m)) / s);
    }
}

template <int TE>
__global__ void __launch_bounds__(TAP_BLOCK) k_dqn_pick(DqnArgs a)
{
    extern __shared__ float4 dqn_lds4[];                                       // (float4: the 16-byte reads need the base aligned)
    dqn_step<TE>(a, reinterpret_cast<float *>(dqn_lds4), (int)blockIdx.x * TE, threadIdx.x);
}

template <int TE> int dqn_launch(tap_ctx *ctx, const DqnArgs &a, hipStream_t st)
{
    const size_t lds = dqn_lds_bytes(TE, a.w.P);
    if (lds > tap_lds_limit(ctx))
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "pack-net pick: %zu bytes of LDS per workgroup, the device allows %zu", lds, tap_lds_limit(ctx));
    TAP_HIP_CHECK(ctx, tap_allow_lds(k_dqn_pick<TE>, lds));
    hipLaunchKernelGGL(k_dqn_pick<TE>, dim3((unsigned)((a.B + TE - 1) / TE)), dim3(TAP_BLOCK), lds, st, a);
    TAP_LAUNCH_CHECK(ctx, "k_dqn_pick");
    tap_variant_hit(ctx, TAP_HIT_DQN, 2, TE, TapVariant{a.w.Wm != a.w.W ? 1 : 0, a.w.P, 0}, 0);
    return TAP_OK;
}

} // namespace

extern "C" int tap_dqn_pick_geometry(int W, int Wm, int32_t *out)
{
    const int P = Wm + 2;
    if (W < 2 || (Wm != W && Wm != W - 1) || P > DQN_PMAX) return TAP_E_UNSUPPORTED;
    if (out) { out[0] = dqn_te(P); out[1] = P; out[2] = (int32_t)dqn_lds_bytes(dqn_te(P), P); }
    return TAP_OK;
}

extern "C" int tap_dqn_pick(tap_ctx *ctx, const tap_dqn_weights *w, const float *pnet, int pnet_stride, const float *block,
                            int block_stride, int B, int64_t *x_out, float *logp_out, float *probs_out, void *stream)
{
    if (!w) return tap_fail(ctx, TAP_E_INVALID, "pack-net pick: null weights");
    if (B < 0 || w->W < 1 || (w->Wm != w->W && w->Wm != w->W - 1) || w->P != w->Wm + 2)
        return tap_fail(ctx, TAP_E_INVALID, "pack-net pick: B %d, weights of W %d, Wm %d, P %d (needs Wm = W or W - 1, P = Wm + 2)", B, w->W,
                        w->Wm, w->P);
    if (B == 0) return TAP_OK; // an empty batch has no buffers to check
    if (!pnet || !block || !x_out || !logp_out || !w->c1 || !w->W2p || !w->b2 || !w->W3p || !w->b3 || !w->L1p || !w->l1b || !w->head_w ||
        !w->head_b)
        return tap_fail(ctx, TAP_E_INVALID, "pack-net pick: null buffer");
    if (pnet_stride < w->Wm || block_stride < 2)
        return tap_fail(ctx, TAP_E_INVALID, "pack-net pick: env strides %d / %d floats for %d map entries and 2 sides", pnet_stride, block_stride, w->Wm);
    if (tap_dqn_pick_geometry(w->W, w->Wm, nullptr) != TAP_OK)
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "pack-net pick: W %d with %d positions (needs 2 <= W and at most %d positions)", w->W, w->P, DQN_PMAX);
    const void *f32[] = {pnet, block, logp_out, probs_out};
    const void *b16[] = {w->c1, w->W2p, w->b2, w->W3p, w->b3, w->L1p, w->l1b, w->head_w, w->head_b};   // read 16 bytes at a time
    bool bad = (reinterpret_cast<uintptr_t>(x_out) & 7) != 0;
    for (const void *p : f32) bad = bad || (reinterpret_cast<uintptr_t>(p) & 3) != 0;
    for (const void *p : b16) bad = bad || (reinterpret_cast<uintptr_t>(p) & 15) != 0;
    if (bad)
        return tap_fail(ctx, TAP_E_INVALID, "pack-net pick: every weight buffer must be 16-byte aligned, x_out 8-byte, the other buffers 4-byte");
    DqnArgs a = {};
    a.w = *w;
    a.pnet = pnet; a.block = block;
    a.pnet_stride = pnet_stride; a.block_stride = block_stride; a.B = B;
    a.x = x_out; a.logp = logp_out; a.probs = probs_out;
    return dqn_te(w->P) == 16 ? dqn_launch<16>(ctx, a, (hipStream_t)stream) : dqn_launch<8>(ctx, a, (hipStream_t)stream);
}
