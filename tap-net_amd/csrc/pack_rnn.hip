// pack_rnn.hip -- the global pack-net's forward in ONE launch (pack_net/LG_RL.py: PackRNN.forward, LG_RL.py:603-675, eval
// form; tapenv.h: tap_pack_rnn_forward has the contract): the encoder GRU over the T blocks, then blocks_num decoder
// steps, each height-map input -> GRU cell -> fc -> softmax -> first maximum -> PackEngine.step, for all B envs.  An
// env's forward depends on no other env, so nothing leaves the workgroup between the steps: the hidden states, the
// constant part of the decoder's input, the logits and the container's height-map live in the LDS, the counters and
// the error word in registers, and the blob is written once at the end (the tape: one row per step).
//
// Geometry: k_decoder_step's (decoder.hip).  A workgroup takes DEC_TE = 16 consecutive envs, a wavefront DEC_E = 4 of
// them, a lane one hidden row j of a 64-row chunk and its three gates; the weights stream through the LDS in (64 rows x
// gates) x (DEC_KC = 32 terms) blocks, the hidden chunk outermost, the sums in registers across the term blocks; the
// cell is tap_decoder.h's dec_cell, called with an argument struct of B = 0 so that it writes the h' tile only.  Every
// tile row -- h, h', a = relu(fc.0 h'), the input x, the logits, the height-map -- is read and written by the wavefront
// that owns the env: the workgroup's barriers only guard the weight block.  What is new against k_decoder_step: the
// loops over t and i inside the launch (the two h tiles swap roles after each step), D = 384 = 6 chunks for LG, the fc
// head (fc.0 with one row per lane on the h' tile, its result into the dead old-h tile; fc.2 with lane c = column c),
// and the pick and the engine step per env with a lane per column (k_place_at's rules, engine mode: place_at.hip).
//
// LDS, floats: weight block 192 x 36 | x tile 16 x 64 (later the fp64 softmax terms) | two h tiles 16 x D | u 16 x 3 D |
// height-map 16 x 64 ints: 115 KB for G, 155 KB for LG -- one workgroup per CU, one wavefront per SIMD.  Nothing else on
// the CU hides this workgroup's latencies, so the weight block is loaded one block ahead of the multiply-adds (prn_load /
// prn_store, 16 bytes per lane), fc takes three term blocks per barrier pair, and whole blocks are multiplied by an
// unrolled copy of dec_mac (prn_mac): the same operations in the same order.  DESIGN.md 7p has the figures.
//
// Every sum is ONE chain of fmaf in ascending term order and nothing crosses an env: two calls give the same bytes and
// an env's bytes do not depend on the batch or the tile around it.  The only cross-lane operations are the maximum of
// the logits / of the footprint (order-free), two ballots, and the integer sums of the height-map.
#include "tap_bitshadow.h"
#include "tap_decoder.h"
#include "tap_place.h"

namespace {

constexpr int TAP_HIT_PACK_RNN = 32;        // launch record (tapenv.h: tap_variant_hits), after critic.hip's 31
constexpr int PRN_HB = 128;                 // block_hidden_size = height_hidden_size, the only shape load_pack_net builds
constexpr int PRN_XS = 64;                  // row stride of the x / logit / height-map tiles: W <= 64

struct PrnArgs {
    tap_env_desc d;
    EnvView v;
    tap_pack_rnn_weights w;
    const float *blocks;                    // (B, 2, T)
    int T, n, max_blocks;
    float *logp, *reward, *feature;         // (B, n), (B,), (B, W') or null
};

inline size_t prn_lds_bytes(int D)
{
    return ((size_t)DEC_WROWS * DEC_WS + 2 * (size_t)DEC_TE * PRN_XS + 5 * (size_t)DEC_TE * D) * sizeof(float);
}

// One weight block on its way to the LDS, in two halves, so that the global loads of block k + 1 are in flight while block k
// is multiplied: lw[(s * 64 + r) * DEC_WS + k] = W[(s * gstride + row0 + r) * ld + k0 + s * kstride + k] for s < NG, r < 64,
// k < DEC_KC; zeros for a row r >= nrows and a term s * kstride + k >= kn.  kstride = 0: dec_fill_weights' block (64 hidden
// rows x their NG gates, gstride rows apart); gstride = 0, kstride = DEC_KC: 64 rows x NG consecutive term blocks (fc.0, fc.2).
template <int NG> struct PrnBlock {
    float v[NG * 64 * DEC_KC / TAP_BLOCK];
};
// VEC: 16-byte loads and LDS stores, a lane four consecutive terms -- for the matrices whose rows are a multiple of four terms
// long (every one but Pd_h, W' terms); the entry point requires 16-byte aligned weight buffers.  kn is then a multiple of 4.
template <int NG, bool VEC>
__device__ __forceinline__ void prn_load(PrnBlock<NG> &b, const float *W, int ld, int gstride, int kstride, int row0, int nrows, int k0, int kn, int tid)
{
    if constexpr (VEC) {
#pragma unroll
        for (int it = 0; it < NG * 64 * DEC_KC / (4 * TAP_BLOCK); ++it) {
            const int i = it * TAP_BLOCK + tid, r = i / (DEC_KC / 4), k = 4 * (i - r * (DEC_KC / 4)), sb = r >> 6, rr = r & 63, kk = sb * kstride + k;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kk < kn && rr < nrows) q = *reinterpret_cast<const float4 *>(W + (unsigned)((sb * gstride + row0 + rr) * ld + k0 + kk));
            b.v[4 * it] = q.x; b.v[4 * it + 1] = q.y; b.v[4 * it + 2] = q.z; b.v[4 * it + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int it = 0; it < NG * 64 * DEC_KC / TAP_BLOCK; ++it) {
            const int i = it * TAP_BLOCK + tid, r = i / DEC_KC, k = i - r * DEC_KC, sb = r >> 6, rr = r & 63, kk = sb * kstride + k;
            b.v[it] = (kk < kn && rr < nrows) ? W[(unsigned)((sb * gstride + row0 + rr) * ld + k0 + kk)] : 0.f;
        }
    }
}
template <int NG, bool VEC> __device__ __forceinline__ void prn_store(float *lw, const PrnBlock<NG> &b, int tid)
{
    if constexpr (VEC) {
#pragma unroll
        for (int it = 0; it < NG * 64 * DEC_KC / (4 * TAP_BLOCK); ++it) {
            const int i = it * TAP_BLOCK + tid, r = i / (DEC_KC / 4), k = 4 * (i - r * (DEC_KC / 4));
            *reinterpret_cast<float4 *>(lw + r * DEC_WS + k) = make_float4(b.v[4 * it], b.v[4 * it + 1], b.v[4 * it + 2], b.v[4 * it + 3]);
        }
    } else {
#pragma unroll
        for (int it = 0; it < NG * 64 * DEC_KC / TAP_BLOCK; ++it) {
            const int i = it * TAP_BLOCK + tid, r = i / DEC_KC, k = i - r * DEC_KC;
            lw[r * DEC_WS + k] = b.v[it];
        }
    }
}

// dec_mac over one whole block of DEC_KC terms, the same multiply-adds in the same order, unrolled: a workgroup here is alone
// on its CU (one wavefront per SIMD), so the LDS reads of the next terms must be in flight behind this wavefront's own
// multiply-adds -- nobody else hides them
template <int NG>
__device__ __forceinline__ void prn_mac(const float *lw, const float *act, int astride, int lane, float (&acc)[NG][DEC_E])
{
#pragma unroll 4
    for (int k4 = 0; k4 < DEC_KC / 4; ++k4) {
        float4 w[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) w[g] = *reinterpret_cast<const float4 *>(lw + (g * 64 + lane) * DEC_WS + 4 * k4);
#pragma unroll
        for (int e = 0; e < DEC_E; ++e) {
            const float4 x = *reinterpret_cast<const float4 *>(act + e * astride + 4 * k4);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                float s = acc[g][e];
                s = fmaf(w[g].x, x.x, s);
                s = fmaf(w[g].y, x.y, s);
                s = fmaf(w[g].z, x.z, s);
                s = fmaf(w[g].w, x.w, s);
                acc[g][e] = s;
            }
        }
    }
}

// acc[g][e] += sum_k W[g * gstride + row0 + lane][k] act[e][k] over K terms, the chain in ascending k: blocks of DEC_KC terms
// through lw, the next block's loads issued before this block's multiply-adds.  Every lane of the workgroup calls it.
template <bool VEC>
__device__ __forceinline__ void prn_gates(float *lw, const float *W, int ld, int gstride, int row0, int K, const float *act, int astride, int lane,
                                          int tid, float (&acc)[3][DEC_E])
{
    PrnBlock<3> blk;
    prn_load<3, VEC>(blk, W, ld, gstride, 0, row0, 64, 0, min(DEC_KC, K), tid);
    for (int k0 = 0; k0 < K; k0 += DEC_KC) {
        const int kn = min(DEC_KC, K - k0);
        __syncthreads();                                                   // the previous block has been consumed
        prn_store<3, VEC>(lw, blk, tid);
        __syncthreads();
        if (k0 + DEC_KC < K) prn_load<3, VEC>(blk, W, ld, gstride, 0, row0, 64, k0 + DEC_KC, min(DEC_KC, K - k0 - DEC_KC), tid);
        if (kn == DEC_KC) prn_mac<3>(lw, act + k0, astride, lane, acc);
        else dec_mac<3>(lw, act + k0, astride, (kn + 3) >> 2, lane, acc);
    }
}
// the same for one row per lane (rows row0 + lane < row0 + nrows of a matrix of K = a multiple of DEC_KC terms), three term
// blocks per pass
__device__ __forceinline__ void prn_rows(float *lw, const float *W, int ld, int row0, int nrows, int K, const float *act, int astride, int lane,
                                         int tid, float (&acc)[1][DEC_E])
{
    PrnBlock<3> blk;
    prn_load<3, true>(blk, W, ld, 0, DEC_KC, row0, nrows, 0, min(3 * DEC_KC, K), tid);
    for (int k0 = 0; k0 < K; k0 += 3 * DEC_KC) {
        const int kn = min(3 * DEC_KC, K - k0);
        __syncthreads();
        prn_store<3, true>(lw, blk, tid);
        __syncthreads();
        if (k0 + 3 * DEC_KC < K) prn_load<3, true>(blk, W, ld, 0, DEC_KC, row0, nrows, k0 + 3 * DEC_KC, min(3 * DEC_KC, K - k0 - 3 * DEC_KC), tid);
        for (int sb = 0; sb * DEC_KC < kn; ++sb)
            prn_mac<1>(lw + sb * 64 * DEC_WS, act + k0 + sb * DEC_KC, astride, lane, acc);
    }
}

// entry c of the net's input from a height-map row (LG_RL.py:498-515): full, zero (minus the minimum) or diff; 0 past W'
__device__ __forceinline__ float prn_input(const int *hm, int form, int W, int c)
{
    if (form == TAP_FEAT_ZERO) {
        const int mn = tap_wave_min(c < W ? hm[c] : INT_MAX);
        return c < W ? (float)(hm[c] - mn) : 0.f;
    }
    if (form == TAP_FEAT_DIFF) return c < W - 1 ? (float)(hm[c + 1] - hm[c]) : 0.f;
    return c < W ? (float)hm[c] : 0.f;
}

// KIND 0 = G (D = 256), 1 = LG (D = 384: the block's own two sides join the decoder's input)
template <int KIND>
__global__ void __launch_bounds__(TAP_BLOCK) k_pack_rnn_forward(PrnArgs a)
{
    constexpr int D = KIND ? 3 * PRN_HB : 2 * PRN_HB, HB = PRN_HB;
    extern __shared__ float4 prn_lds4[];                                   // (float4: the 16-byte reads need the base aligned)
    float *lw = reinterpret_cast<float *>(prn_lds4), *xa = lw + DEC_WROWS * DEC_WS, *hA = xa + DEC_TE * PRN_XS;
    float *hB = hA + DEC_TE * D, *u = hB + DEC_TE * D;
    int *s_hm = reinterpret_cast<int *>(u + DEC_TE * 3 * D);
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX();
    const int B = a.d.B, W = a.d.W, form = a.w.form, Wp = W - (form == TAP_FEAT_DIFF ? 1 : 0);
    const int T = a.T, n = a.n, mb = a.max_blocks;
    const int e0 = (int)blockIdx.x * DEC_TE, ew = wave * DEC_E;
    const bool incol = lane < W;
    const tap_pack_rnn_weights &w = a.w;
    // dec_cell with B = 0: the h' tile only, no store to global memory
    DecCellArgs cell_e = {}, cell_d = {};
    cell_e.Hd = HB;
    cell_d.Hd = D;
    const DecSeed seed = {0, 0, 0};
    const float *bp[DEC_E];                                                // blocks[b, 0, :] (an env past the batch reads the last one's)
#pragma unroll
    for (int e = 0; e < DEC_E; ++e) bp[e] = a.blocks + (size_t)min(e0 + ew + e, B - 1) * 2 * T;

    // ---- encoder: h_e over all T columns -------------------------------------------------------------------------------
    float *hl = hA, *hn = hA + DEC_TE * HB;
    for (int i = tid; i < DEC_TE * HB; i += TAP_BLOCK) hl[i] = 0.f;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        float bx[DEC_E], by[DEC_E];
#pragma unroll
        for (int e = 0; e < DEC_E; ++e) { bx[e] = bp[e][t]; by[e] = bp[e][T + t]; }
        for (int jc = 0; jc < HB / 64; ++jc) {
            const int j = jc * 64 + lane;
            float gi[3][DEC_E], gh[3][DEC_E];
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const int row = g * HB + j;
                const float c = w.ce[row], p0 = w.Pe[2 * row], p1 = w.Pe[2 * row + 1], bi = w.enc_b_hh[row];
#pragma unroll
                for (int e = 0; e < DEC_E; ++e) { gi[g][e] = fmaf(p1, by[e], fmaf(p0, bx[e], c)); gh[g][e] = bi; }
            }
            if (t > 0) prn_gates<true>(lw, w.enc_w_hh, HB, HB, jc * 64, HB, hl + ew * HB, HB, lane, tid, gh);
            dec_cell(cell_e, seed, gi, gh, hl, hn, e0, ew, jc, lane);
        }
        __syncthreads();
        float *s = hl; hl = hn; hn = s;
    }
    // ---- u: the constant part of the decoder's input, from cd over the HB terms of enc = hl ------------------------------
    for (int jc = 0; jc < D / 64; ++jc) {
        const int j = jc * 64 + lane;
        float acc[3][DEC_E];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const float c = w.cd[g * D + j];
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) acc[g][e] = c;
        }
        prn_gates<true>(lw, w.Pd_e, HB, D, jc * 64, HB, hl + ew * HB, HB, lane, tid, acc);
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) u[(ew + e) * 3 * D + g * D + j] = acc[g][e];
    }
    __syncthreads();
    // ---- decoder: h_d = 0, the empty container ---------------------------------------------------------------------------
    hl = hA;
    hn = hB;
    for (int i = tid; i < DEC_TE * D; i += TAP_BLOCK) hl[i] = 0.f;
    for (int i = tid; i < DEC_TE * PRN_XS; i += TAP_BLOCK) s_hm[i] = 0;
    __syncthreads();
    int valid[DEC_E], empty[DEC_E], nstab[DEC_E], err[DEC_E];              // the same on every lane of the wavefront
#pragma unroll
    for (int e = 0; e < DEC_E; ++e) valid[e] = empty[e] = nstab[e] = err[e] = 0;
    double *sd = reinterpret_cast<double *>(xa + ew * PRN_XS);             // 64 fp64 terms in the wavefront's own x rows

    for (int i = 0; i < n; ++i) {
        // engine: `start` = the container is empty before this step, `wrap` = it is cleared after it (place_at.hip)
        const bool start = mb > 0 ? i % mb == 0 : i == 0;
        const bool wrap = mb > 0 && (i + 1) % mb == 0;
        float bx[DEC_E], by[DEC_E];
#pragma unroll
        for (int e = 0; e < DEC_E; ++e) {
            bx[e] = bp[e][i];
            by[e] = bp[e][T + i];
            xa[(ew + e) * PRN_XS + lane] = prn_input(s_hm + (ew + e) * PRN_XS, form, W, lane);
        }
        for (int jc = 0; jc < D / 64; ++jc) {
            const int j = jc * 64 + lane;
            float gi[3][DEC_E], gh[3][DEC_E];
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const int row = g * D + j;
                const float bi = w.dec_b_hh[row];
                float p0 = 0.f, p1 = 0.f;
                if (KIND) { p0 = w.Pd_b[2 * row]; p1 = w.Pd_b[2 * row + 1]; }
#pragma unroll
                for (int e = 0; e < DEC_E; ++e) {
                    float s = u[(ew + e) * 3 * D + row];
                    if (KIND) s = fmaf(p1, by[e], fmaf(p0, bx[e], s));
                    gi[g][e] = s;
                    gh[g][e] = bi;
                }
            }
            prn_gates<false>(lw, w.Pd_h, Wp, D, jc * 64, Wp, xa + ew * PRN_XS, PRN_XS, lane, tid, gi);
            if (i > 0) prn_gates<true>(lw, w.dec_w_hh, D, D, jc * 64, D, hl + ew * D, D, lane, tid, gh);
            dec_cell(cell_d, seed, gi, gh, hl, hn, e0, ew, jc, lane);
        }
        // a = relu(fc.0 h') into the old h tile, which nothing reads any more
        for (int jc = 0; jc < D / 64; ++jc) {
            const int j = jc * 64 + lane;
            float acc[1][DEC_E];
            const float c = w.fc0_b[j];
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) acc[0][e] = c;
            prn_rows(lw, w.fc0_w, D, jc * 64, 64, D, hn + ew * D, D, lane, tid, acc);
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) hl[(ew + e) * D + j] = acc[0][e] > 0.f ? acc[0][e] : 0.f;
        }
        // l_c = fc.2 a, lane c
        float l[1][DEC_E];
        {
            const float c = incol ? w.fc2_b[lane] : 0.f;
#pragma unroll
            for (int e = 0; e < DEC_E; ++e) l[0][e] = c;
            prn_rows(lw, w.fc2_w, D, 0, W, D, hl + ew * D, D, lane, tid, l);
        }
        // the pick and the engine step, env by env, a lane per column
#pragma unroll
        for (int e = 0; e < DEC_E; ++e) {
            const int b = e0 + ew + e;
            const bool ev = b < B;
            const float lv = l[0][e];
            const float m = tap_wave_max(incol ? lv : -INFINITY);
            const u64 top = __ballot(incol && lv == m);
            const int pick = top ? __ffsll((long long)top) - 1 : 0;            // the first maximum (LG_RL.py:659)
            tap_wave_lds_sync();                                               // the x rows / the previous env's terms have been read
            sd[lane] = incol ? exp((double)(lv - m)) : 0.0;
            tap_wave_lds_sync();
            double ssum = 0.0;
            for (int c = 0; c < W; ++c) ssum += sd[c];
            const float lp = (float)(-log(ssum));                              // log of the largest probability (LG_RL.py:654)
            // PackEngine.step at column `pick`: k_place_at<64, true, true>'s rules
            int *hrow = s_hm + (ew + e) * PRN_XS;
            if (start) valid[e] = empty[e] = nstab[e] = 0;
            if (i == 0) err[e] = 0;
            const int bw = (int)bx[e], bh = (int)by[e];                        // block.int() (LG_RL.py:450)
            bool do_step = true;
            int er = 0;
            if (bw < 1 || bh < 1) { er |= 4; do_step = false; }
            const int xl = min(pick, W - bw);
            if (do_step && xl < 0) { er |= 4; do_step = false; }               // block wider than W
            const int x = do_step ? xl : 0, wd = do_step ? bw : 0;
            const bool inb = incol && lane >= x && lane < x + wd;
            const int hm0 = incol ? hrow[lane] : 0;
            const int z = tap_wave_max(inb ? hm0 : 0);
            const u64 wave_eq = __ballot(inb && hm0 == z);
            int hm = hm0, stab = 1;
            if (do_step) {
                if (inb) hm = z + bh;
                if (z > 0) {
                    const u64 eq = (wave_eq >> x) & (wd >= 64 ? ~0ull : ((1ull << wd) - 1ull));
                    stab = tap_stable2d(wd, eq);
                }
                if (z + bh > a.d.H) er |= 1;                                   // the reference clips silently
            }
            const int hsum = tap_wave_sum(incol ? hm : 0), hmax = tap_wave_max(incol ? hm : 0);
            if (do_step) {
                valid[e] += bw * bh;
                nstab[e] += stab;
                empty[e] = hsum - valid[e];
            }
            err[e] |= er;
            if (ev && lane == 0) {
                int32_t *q = a.v.pos + (size_t)i * 2 * B + b;
                q[0] = x;                                                      // (0, 0), unstable, for a refused step
                q[B] = z;
                a.v.stable[(size_t)i * B + b] = (uint8_t)(do_step ? stab : 0);
                a.logp[(size_t)b * n + i] = lp;
                if (i == n - 1) {                                              // LG_RL.py:460-475, rw.astype('float32')
                    const int since = (mb > 0 ? i % mb : i) + 1;
                    const double box = (double)hmax * W, ve = (double)valid[e] + (double)empty[e];
                    const double C = box == 0 ? 0.0 : (double)valid[e] / box;
                    const double P = ve == 0 ? 0.0 : (double)valid[e] / ve;
                    const double S = (double)nstab[e] / (double)since;
                    a.reward[b] = (float)(((C + P) + S) / 3);
                }
            }
            hrow[lane] = (wrap || !incol) ? 0 : hm;                            // what the blob and the next input see
            if (wrap) valid[e] = empty[e] = nstab[e] = 0;
        }
        __syncthreads();
        float *s = hl; hl = hn; hn = s;
    }
    // ---- the blob, once ------------------------------------------------------------------------------------------------
#pragma unroll
    for (int e = 0; e < DEC_E; ++e) {
        const int b = e0 + ew + e;
        const int *hrow = s_hm + (ew + e) * PRN_XS;
        const float xin = prn_input(hrow, form, W, lane);                      // (a wave-wide minimum: every lane takes part)
        if (b < B) {
            if (incol) a.v.hm[(size_t)b * W + lane] = hrow[lane];
            if (a.feature && lane < Wp) a.feature[(size_t)b * Wp + lane] = xin;
            if (lane == 0) {
                reinterpret_cast<int4 *>(a.v.cnt)[b] = make_int4(valid[e], empty[e], nstab[e], n);
                a.v.err[b] = err[e];
            }
        }
    }
}

template <int KIND> int prn_launch(tap_ctx *ctx, const PrnArgs &a, hipStream_t st)
{
    constexpr int D = KIND ? 3 * PRN_HB : 2 * PRN_HB;
    const size_t lds = prn_lds_bytes(D);
    if (lds > tap_lds_limit(ctx))
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "pack-net forward: %zu bytes of LDS per workgroup, the device allows %zu", lds, tap_lds_limit(ctx));
    TAP_HIP_CHECK(ctx, tap_allow_lds(k_pack_rnn_forward<KIND>, lds));
    hipLaunchKernelGGL(k_pack_rnn_forward<KIND>, dim3((unsigned)((a.d.B + DEC_TE - 1) / DEC_TE)), dim3(TAP_BLOCK), lds, st, a);
    TAP_LAUNCH_CHECK(ctx, "k_pack_rnn_forward");
    tap_variant_hit(ctx, TAP_HIT_PACK_RNN, 2, DEC_TE, TapVariant{KIND, D / 64, 0}, 0);
    return TAP_OK;
}

} // namespace

extern "C" int tap_pack_rnn_forward(tap_ctx *ctx, const tap_env_desc *d, void *state, const float *blocks, int T, int blocks_num,
                                    int max_blocks, const tap_pack_rnn_weights *w, float *logp_out, float *reward_out,
                                    float *feature_out, void *stream)
{
    if (!d || !w) return tap_fail(ctx, TAP_E_INVALID, "pack-net forward: null descriptor or weights");
    if (tap_place_at_semantics(d) != TAP_AT_NET || d->D != 2)
        return tap_fail(ctx, TAP_E_INVALID, "pack-net forward: needs a TAP_AT_NET descriptor (tap_env_desc_set_place_at)");
    if (T < 1 || blocks_num < 1 || blocks_num > T || max_blocks < 0)
        return tap_fail(ctx, TAP_E_INVALID, "pack-net forward: blocks_num %d of T = %d columns, max_blocks %d", blocks_num, T, max_blocks);
    const int rc = tap_desc_validate(ctx, d);
    if (rc) return rc;
    if (d->B == 0) return TAP_OK; // an empty batch has no buffers to check
    const bool lg = w->kind == TAP_PACK_LG;
    if (!state || !blocks || !logp_out || !reward_out || !w->Pe || !w->ce || !w->enc_w_hh || !w->enc_b_hh || !w->Pd_e || (lg && !w->Pd_b) ||
        !w->Pd_h || !w->cd || !w->dec_w_hh || !w->dec_b_hh || !w->fc0_w || !w->fc0_b || !w->fc2_w || !w->fc2_b)
        return tap_fail(ctx, TAP_E_INVALID, "pack-net forward: null buffer");
    if (w->W != d->W) return tap_fail(ctx, TAP_E_INVALID, "pack-net forward: weights for W = %d, a descriptor of W = %d", w->W, d->W);
    if ((w->kind != TAP_PACK_G && w->kind != TAP_PACK_LG) || w->Hb != PRN_HB || w->Hh != PRN_HB || d->W < 2 || d->W > 64 ||
        (w->form != TAP_FEAT_FULL && w->form != TAP_FEAT_ZERO && w->form != TAP_FEAT_DIFF) || T > d->n_max)
        return tap_fail(ctx, TAP_E_UNSUPPORTED,
                        "pack-net forward: kind %d, Hb %d, Hh %d, W %d, form %d, T %d on a tape of %d (needs G or LG, Hb = Hh = 128, 2 <= W <= 64, "
                        "a TAP_FEAT_* form, T within the tape)", w->kind, w->Hb, w->Hh, d->W, w->form, T, d->n_max);
    const void *f32[] = {blocks, logp_out, reward_out, feature_out};
    const void *b16[] = {state, w->Pe, w->ce, w->enc_w_hh, w->enc_b_hh, w->Pd_e, w->Pd_b, w->Pd_h, w->cd, w->dec_w_hh, w->dec_b_hh, w->fc0_w,
                         w->fc0_b, w->fc2_w, w->fc2_b};                      // the weight blocks are read 16 bytes at a time
    bool bad = false;
    for (const void *p : f32) bad = bad || dec_misaligned(p);
    for (const void *p : b16) bad = bad || (reinterpret_cast<uintptr_t>(p) & 15) != 0;
    if (bad)
        return tap_fail(ctx, TAP_E_INVALID, "pack-net forward: the state blob and every weight buffer must be 16-byte aligned, the other buffers 4-byte");
    PrnArgs a = {};
    a.d = *d;
    tap_env_layout(d, state, &a.v);
    a.w = *w;
    a.blocks = blocks;
    a.T = T; a.n = blocks_num; a.max_blocks = max_blocks;
    a.logp = logp_out; a.reward = reward_out; a.feature = feature_out;
    return lg ? prn_launch<1>(ctx, a, (hipStream_t)stream) : prn_launch<0>(ctx, a, (hipStream_t)stream);
}
