// tap_bitshadow.h -- what the kernels on the bit shadow share: pointer.hip, critic.hip and encode.hip all turn a column's
// shadow word into the sum of a few columns of a folded matrix kept in the LDS, and their entries make the same host checks.
// Here, once: the alignment and "needs a bit shadow" predicates, the wavefront butterflies, the masks of the rows in use, the
// [r][x] fill of a chunk of the folded matrix and the scalar loop over the set bits of a word.  Everything is inline or
// __forceinline__ and lives in the including unit's anonymous namespace; the sums keep the order their callers document, so
// the bytes do not depend on where the code stands (DESIGN 7f has the listings, and the pieces that stayed written out).
#pragma once

#include <initializer_list>

#include "tap_common.h"
#include "tap_place.h"   // tap_wave_lds_sync

namespace {

// ---- host ---------------------------------------------------------------------------------------------------------
inline bool tap_misaligned(const void *p, unsigned to) { return ((uintptr_t)p & (to - 1)) != 0; }
using TapPtrList = std::initializer_list<const void *>;
inline bool tap_any_misaligned(TapPtrList ps, unsigned to)
{
    bool bad = false;
    for (const void *p : ps) bad = bad || tap_misaligned(p, to);
    return bad;
}
// a (rows, nR) window has a bit shadow (tap_step_request.h); a shape that is not positive has none
inline bool tap_has_bit_shadow(int rows, int nR) { return rows >= 1 && nR >= 1 && tap_window_has_shadow(rows, nR); }
inline int tap_bit_planes(int rows) { return rows > 64 ? 2 : 1; }

// ---- device -------------------------------------------------------------------------------------------------------
// xor butterflies over the wavefront: every lane ends with the same value
__device__ __forceinline__ float tap_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float tap_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double tap_wave_sum(double v)   // train.hip's norms
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int tap_wave_sum(int v)         // pack_rnn.hip's height-map terms, as the two below
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int tap_wave_max(int v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int tap_wave_min(int v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// bits at positions >= rows are ignored: the masks of each plane's word
__device__ __forceinline__ unsigned long long tap_rows_mask0(int rows) { return rows >= 64 ? ~0ull : (1ull << rows) - 1; }
__device__ __forceinline__ unsigned long long tap_rows_mask1(int rows)
{
    return rows >= 128 ? ~0ull : rows > 64 ? (1ull << (rows - 64)) - 1 : 0ull;
}

// M[x0 + hl][r] -> lw[r * (HC + 1) + hl] for n of a chunk's HC rows from x0: global reads in memory order, LDS writes at
// the odd stride HC + 1.  The caller's barriers stand before (the previous chunk has been consumed) and after.
__device__ __forceinline__ void tap_fill_chunk(const float *M, float *lw, int x0, int HC, int n, int rows, int tid)
{
    const int MS = HC + 1;
    for (int i = tid; i < n * rows; i += TAP_BLOCK) {
        const int hl = i / rows, r = i - hl * rows;
        lw[r * MS + hl] = M[(size_t)x0 * rows + i];
    }
}

// acc[i] += lw[r * stride + lane + 64 i] for the rows r = 32 p + (a set bit of x), ascending; x is wave-uniform, so the loop
// is scalar: one trip per SET row, nothing for an unset one
template <int R>
__device__ __forceinline__ void tap_add_set_rows_piece(const float *lw, int stride, int lane, int p, unsigned x, float (&acc)[R])
{
    while (x) {
        const int r = 32 * p + __builtin_ctz(x);
        x &= x - 1;
        const float *lp = lw + r * stride + lane;
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = acc[i] + lp[i * 64];
    }
}
// the same for a column's (masked, wave-uniform) words: the four 32-bit pieces in ascending rows, plane 0 before plane 1
template <int R>
__device__ __forceinline__ void tap_add_set_rows(const float *lw, int stride, int lane, unsigned long long w0, unsigned long long w1,
                                                 float (&acc)[R])
{
    const unsigned piece[4] = {(unsigned)w0, (unsigned)(w0 >> 32), (unsigned)w1, (unsigned)(w1 >> 32)};
#pragma unroll
    for (int p = 0; p < 4; ++p)
        tap_add_set_rows_piece<R>(lw, stride, lane, p, (unsigned)__builtin_amdgcn_readfirstlane((int)piece[p]), acc);
}

} // namespace
