// tap_pick.h -- the decoding head's device code that more than one unit runs: the fp64 scan, the chunked form's weight
// pass, the log-probability and DRAW's uniform.  policy.hip's kernels (tapenv.h: tap_policy_pick and its forms) are built of
// these, and pointer.hip's fused launch (tap_pointer_pick_static) walks its LDS row of logits with the same functions, so
// that both write the same bytes.  Everything is __forceinline__ and lives in the including unit's anonymous namespace.
#pragma once

#include "tap_common.h"
#include "tap_decoder.h"
#include "tap_place.h"

namespace {

template <int G> __device__ __forceinline__ float group_fmaxf(float v)
{
    group_butterfly<G>((int)(threadIdx.x & 63), [&](auto get) { v = fmaxf(v, __int_as_float(get(__float_as_int(v)))); });
    return v;
}

// inclusive prefix sum of w over the W lowest-aligned lanes that hold `cell` (fp64: shuffle-up on the two halves)
template <int W> __device__ __forceinline__ double scan_up(double w, int cell)
{
    double cum = w;
#pragma unroll
    for (int d = 1; d < W; d <<= 1) {
        const double up = __shfl_up(cum, d, W);
        if (cell >= d) cum += up;
    }
    return cum;
}

__device__ __forceinline__ double wave_read(double v, int lane)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

__device__ __forceinline__ float pick_logp(bool any, float l_ptr, float m, double S)
{
    return any ? (float)(((double)l_ptr - (double)m) - log(S)) : __builtin_nanf("");
}

// one 64-column chunk of the weight pass: this lane's weight and the row's inclusive prefix sum up to its column
struct Chunk {
    bool inr, sel;
    float l;
    double w, cum;
};
__device__ __forceinline__ Chunk pick_chunk(const float *lrow, const float *mrow, int base, int lane, int nR, float m, double &run)
{
    Chunk c;
    const int col = base + lane, at = min(col, nR - 1);
    const float l_raw = lrow[at], mv = mrow[at];
    c.inr = col < nR;
    c.sel = c.inr && mv != 0.f;
    c.l = c.sel ? l_raw : -__builtin_huge_valf();
    c.w = c.sel ? exp((double)c.l - (double)m) : 0.0;
    c.cum = run + scan_up<64>(c.w, lane);
    run = wave_read(c.cum, 63);
    return c;
}

// the uniform of env b of a DRAW call: Philox4x32-10 (tap_decoder.h) at counter (env_offset + b, 0xFFFFFFFF, step, episode mod
// 2^32) -- a hidden row no dropout launch has -- and key (seed mod 2^32, seed >> 32); u = (word0 >> 8) 2^-24, exact in fp32.
// A: a kernel's argument struct with `const long long *state` (the int64[2] (seed, episode) on the device) and the
// unsigned `step` and `env_offset`
template <class A> __device__ __forceinline__ float draw_uniform(const A &a, size_t env)
{
    const unsigned long long seed = (unsigned long long)a.state[0];
    const unsigned episode = (unsigned)(unsigned long long)a.state[1];
    const uint2 w = dec_philox2(a.env_offset + (unsigned)env, 0xFFFFFFFFu, a.step, episode, (unsigned)seed, (unsigned)(seed >> 32));
    return (float)(w.x >> 8) * 5.9604644775390625e-8f;
}

} // namespace
