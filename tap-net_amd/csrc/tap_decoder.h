// tap_decoder.h -- what the decoder-step kernels share (decoder.hip: k_decoder_step; heightmap.hip: k_decoder_step_hm): the
// tile geometry, the weight-block fill and the multiply-accumulate of a (64 rows x NG gates) x (DEC_E envs) register
// tile.  decoder.hip's opening comment describes the geometry.
#pragma once
#include "tap_common.h"

#include <type_traits>

namespace {

constexpr int DEC_E = 4;                    // envs per wavefront
constexpr int DEC_TE = (TAP_BLOCK / 64) * DEC_E;   // envs per workgroup
constexpr int DEC_KC = 32;                  // terms per weight block
constexpr int DEC_WS = DEC_KC + 4;          // row stride of the weight block in the LDS, floats
constexpr int DEC_WROWS = 3 * 64;           // rows of the largest weight block: 64 hidden rows x 3 gates
static_assert((64 * DEC_KC) % TAP_BLOCK == 0 && (DEC_TE * DEC_KC) % TAP_BLOCK == 0, "the fills' trip counts are fixed");

// rows [g * gstride + row0 + (0 .. 63)] for g < NG, terms [k0, k0 + kn) of a row-major matrix of row length ld ->
// lw[(g * 64 + r) * DEC_WS + k], zeros up to DEC_KC.  Global reads along the rows, LDS writes of a 32-lane half on 32
// consecutive banks.  The caller's barriers stand before (the previous block has been consumed) and after.
template <int NG>
__device__ __forceinline__ void dec_fill_weights(float *lw, const float *W, int ld, int gstride, int row0, int k0, int kn, int tid)
{
    constexpr int N = NG * 64 * DEC_KC / TAP_BLOCK;                        // a fixed trip count: the loads of a block are all
    float v[N];                                                            // issued before the first LDS write waits for one
#pragma unroll
    for (int it = 0; it < N; ++it) {
        const int i = it * TAP_BLOCK + tid, r = i / DEC_KC, k = i - r * DEC_KC;
        const int row = (r >> 6) * gstride + row0 + (r & 63);
        v[it] = k < kn ? W[(unsigned)(row * ld + k0 + k)] : 0.f;              // (a weight matrix has at most 3 * 256 * 272 elements)
    }
#pragma unroll
    for (int it = 0; it < N; ++it) {
        const int i = it * TAP_BLOCK + tid, r = i / DEC_KC, k = i - r * DEC_KC;
        lw[r * DEC_WS + k] = v[it];
    }
}

// acc[g][e] = fmaf(w[g][k], act[e][k], acc[g][e]) over 4 * k4n terms in ascending order
template <int NG>
__device__ __forceinline__ void dec_mac(const float *lw, const float *act, int astride, int k4n, int lane, float (&acc)[NG][DEC_E])
{
    for (int k4 = 0; k4 < k4n; ++k4) {
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

__device__ __forceinline__ float dec_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

inline bool dec_hd_ok(int Hd) { return Hd == 64 || Hd == 128 || Hd == 256; }
inline bool dec_misaligned(const void *p) { return ((uintptr_t)p & 3) != 0; }

// ---- dropout inside the launch (tapenv.h: tap_decoder_step_dropout has the definition) ---------------------------------
// What the dropout form of a step kernel takes beside the plain form's arguments.  state = (seed, episode) lives on the
// device: the launch reads it there, so a captured graph draws new masks on every replay.
struct DecDropArgs {
    const long long *state;                 // int64[2]: seed, episode
    unsigned long long *keep;               // (B, 2, Hd / 64): plane 0 drop_rnn, plane 1 drop_hh; bit j % 64 of word j / 64 = row j kept
    float *rnn_out;                         // (B, Hd) the dropped GRU output (what q was formed from), or null
    unsigned step, env_offset, thr_rnn, thr_hh;   // keep iff word >= thr
    float s_rnn, s_hh;                      // float32(1 / (1 - p))
};

// Philox4x32-10 (Salmon et al., SC'11; the standard constants) -> its output words 0 and 1
__device__ __forceinline__ uint2 dec_philox2(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint2(c0, c1);
}

// the two keep predicates of (env b of the call, hidden row j): counter (env_offset + b, j, step, episode mod 2^32), key
// (seed mod 2^32, seed >> 32); word 0 decides drop_rnn, word 1 drop_hh
__device__ __forceinline__ void dec_keep(const DecDropArgs &d, unsigned seed_lo, unsigned seed_hi, unsigned episode, int b, int j,
                                         bool &keep_rnn, bool &keep_hh)
{
    const uint2 w = dec_philox2(d.env_offset + (unsigned)b, (unsigned)j, d.step, episode, seed_lo, seed_hi);
    keep_rnn = w.x >= d.thr_rnn;
    keep_hh = w.y >= d.thr_hh;
}

// the host side's checks of a dropout launch's own arguments
inline bool dec_drop_null(const void *state, const void *keep) { return !state || !keep; }
inline bool dec_drop_misaligned(const void *state, const void *keep) { return (((uintptr_t)state | (uintptr_t)keep) & 7) != 0; }

} // namespace
