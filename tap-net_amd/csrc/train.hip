// train.hip -- the tail of a training iteration (the reference's trainer.py:216-236) in three launches: the advantage, both
// losses and both gradient seeds (tap_reinforce_losses), then clip_grad_norm_ and Adam.step() for every parameter of
// several modules (tap_clip_adam_norm, tap_clip_adam_apply).  tapenv.h has the contracts; DESIGN 7o the orders below.
//
// Sums.  Every sum of these kernels is a float64 sum in an order fixed by the shape alone: a thread's own items in
// ascending order, then an xor butterfly over the wavefront (offsets 32, 16, .. 1: every lane ends with the same bytes),
// then the workgroup's four wavefronts in ascending order, then -- across workgroups -- the partials in ascending order.
// No floating-point atomic anywhere; the one atomic is the integer ticket by which the last workgroup of
// k_reinforce_losses learns that it is the last.
//
// k_reinforce_losses.  One thread per env, 256 envs per workgroup, ceil(B / 256) workgroups.  adv = reward - est (fp32);
// an env whose reward is not finite has adv = 0, zero seeds, adds nothing to the four sums and counts as flagged.
// seed_logp[b, :] = adv / B; seed_est[b] = (-2 adv) / B; the env's actor term is (double)adv * (the float64 sum of its
// tour_logp row, columns ascending), its critic term (double)adv * (double)adv.  A workgroup leaves five float64
// partials (actor, critic, reward, est, flagged); the workgroup that draws the last ticket adds them in workgroup order,
// divides the first four by B and writes the five floats of the stats row; it puts the ticket back to zero.
//
// k_clip_adam_norm.  One workgroup per chunk of the table.  Thread t owns the quads (runs of four elements) t, t + 256, ..
// of its chunk and adds g^2 in element order; one float64 partial per chunk.  The workgroup of a group's first chunk also
// copies the group's step counter to its snapshot, which is what the second launch reads: the second launch's workgroups
// then never read a word that one of them writes.
//
// k_clip_adam_apply.  One workgroup per chunk.  The group's partials are staged through the LDS 256 at a time and added
// in ascending order by every thread alike; thread 0 then derives, in float64, norm = sqrt(sum), coef = min(1, max_norm /
// (norm + 1e-6)), t = snapshot + 1, bc1 = 1 - beta1^t, step_size = lr / bc1, bc2_sqrt = sqrt(1 - beta2^t), and hands
// them on as floats.  Per element, in fp32 and exactly as written (no contraction; the two fmafs are spelled out):
//     g' = g coef;  m = fmaf(beta1, m, (1 - beta1) g');  v = fmaf(beta2, v, (1 - beta2) (g' g'));
//     p = p - step_size (m / (sqrtf(v) / bc2_sqrt + eps));  g = 0 where the launch zeroes.
// A norm that is not finite skips the group: p, m, v and the counter stay, g is zeroed (where the launch zeroes) and the
// group's skipped word goes up by one.  The first chunk's thread 0 writes the group's norm, counter and skipped word.
//
// Both chunk kernels take a quad as one 16-byte access where all four of the chunk's pointers are 16-byte aligned and the
// quad is whole, and as dwords elsewhere (a parameter that is a view at an odd element offset, the tail of a chunk): the
// element-to-thread map and the order of every sum are the same on both paths, so the bytes do not depend on the path.
#include <cmath>

#include "tap_bitshadow.h"
#include "tap_common.h"

namespace {

constexpr int TR_NW = TAP_BLOCK / 64;

// the workgroup's sum of K values per thread: butterflies, then the wavefronts in ascending order; every thread returns
// with out[k] holding the sums.  red: TR_NW * K doubles of LDS.
template <int K>
__device__ __forceinline__ void tr_block_sum(double (&val)[K], double *red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        val[k] = tap_wave_sum(val[k]);
        if (lane == 0) red[wave * K + k] = val[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = red[k];
#pragma unroll
        for (int w = 1; w < TR_NW; ++w) s = s + red[w * K + k];
        val[k] = s;
    }
    __syncthreads();                                                       // red may be written again
}

__global__ void __launch_bounds__(TAP_BLOCK) k_reinforce_losses(const float *reward, const float *est, const float *logp, int B, int n,
                                                               float *adv_out, float *seed_logp, float *seed_est, float *stats,
                                                               double *part, unsigned *ticket)
{
    __shared__ double red[TR_NW * 5];
    __shared__ unsigned last;
    const int b = (int)blockIdx.x * TAP_BLOCK + (int)threadIdx.x;
    double val[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (b < B) {
        const float r = reward[b], e = est[b];
        const bool ok = isfinite(r);
        const float adv = ok ? r - e : 0.f;
        const float sl = adv / (float)B;
        const float *lp = logp + (size_t)b * n;
        float *sp = seed_logp + (size_t)b * n;
        double row = 0.0;
        for (int k = 0; k < n; ++k) {
            row = row + (double)lp[k];
            sp[k] = sl;
        }
        adv_out[b] = adv;
        seed_est[b] = ok ? (-2.f * adv) / (float)B : 0.f;
        if (ok) {
            val[0] = (double)adv * row;
            val[1] = (double)adv * (double)adv;
            val[2] = (double)r;
            val[3] = (double)e;
        } else {
            val[4] = 1.0;
        }
    }
    tr_block_sum<5>(val, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) part[(size_t)blockIdx.x * 5 + k] = val[k];
        __threadfence();                                                   // the partials before the ticket
        last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();                                                       // the ticket before the others' partials
    if (threadIdx.x < 5) {
        const int k = (int)threadIdx.x;
        double s = 0.0;
        for (unsigned w = 0; w < gridDim.x; ++w) s = s + part[(size_t)w * 5 + k];
        stats[k] = (float)(k < 4 ? s / (double)B : s);
    }
    if (threadIdx.x == 0) *ticket = 0u;                                    // for the next launch on this stream
}

// ---- clip + Adam ----------------------------------------------------------------------------------------------------
struct CaGroup {            // what thread 0 derives for its chunk's group
    float coef, step_size, bc2_sqrt, eps, b1, omb1, b2, omb2, norm;
    int skip;
};

__device__ __forceinline__ bool ca_aligned(const tap_adam_chunk &c)
{
    return ((((uintptr_t)c.param) | ((uintptr_t)c.grad) | ((uintptr_t)c.exp_avg) | ((uintptr_t)c.exp_avg_sq)) & 15) == 0;
}

__global__ void __launch_bounds__(TAP_BLOCK) k_clip_adam_norm(const tap_adam_chunk *table, const int32_t *ranges, int64_t *steps, double *part)
{
    __shared__ double red[TR_NW];
    const tap_adam_chunk c = table[blockIdx.x];
    const bool vec = (((uintptr_t)c.grad) & 15) == 0;
    double val[1] = {0.0};
    for (int q = (int)threadIdx.x; 4 * q < c.count; q += TAP_BLOCK) {
        const int i = 4 * q;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && i + 4 <= c.count) {
            const float4 t = *reinterpret_cast<const float4 *>(c.grad + i);
            g[0] = t.x, g[1] = t.y, g[2] = t.z, g[3] = t.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < c.count) g[k] = c.grad[i + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) val[0] = val[0] + (double)g[k] * (double)g[k];   // (a missing element adds +0)
    }
    tr_block_sum<1>(val, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = val[0];
        if ((int)blockIdx.x == ranges[2 * c.group]) steps[2 * c.group + 1] = steps[2 * c.group];
    }
}

__global__ void __launch_bounds__(TAP_BLOCK) k_clip_adam_apply(const tap_adam_chunk *table, const int32_t *ranges, const double *hyper,
                                                              int64_t *steps, const double *part, float *norms, int32_t *skipped, int zero)
{
    __shared__ double tile[TAP_BLOCK];
    __shared__ CaGroup gs;
    const tap_adam_chunk c = table[blockIdx.x];
    const int first = ranges[2 * c.group], chunks = ranges[2 * c.group + 1];
    double sum = 0.0;
    for (int base = 0; base < chunks; base += TAP_BLOCK) {
        const int m = min(TAP_BLOCK, chunks - base);
        if ((int)threadIdx.x < m) tile[threadIdx.x] = part[first + base + (int)threadIdx.x];
        __syncthreads();
        for (int k = 0; k < m; ++k) sum = sum + tile[k];                   // ascending, the same on every thread
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double *h = hyper + 5 * c.group;                             // lr, beta1, beta2, eps, max_norm
        const double norm = sqrt(sum);
        const int64_t t = steps[2 * c.group + 1] + 1;
        const double bc1 = 1.0 - pow(h[1], (double)t), bc2 = 1.0 - pow(h[2], (double)t);
        gs.skip = isfinite(norm) ? 0 : 1;
        gs.coef = (float)fmin(1.0, h[4] / (norm + 1e-6));
        gs.step_size = (float)(h[0] / bc1);
        gs.bc2_sqrt = (float)sqrt(bc2);
        gs.eps = (float)h[3];
        gs.b1 = (float)h[1], gs.omb1 = (float)(1.0 - h[1]);
        gs.b2 = (float)h[2], gs.omb2 = (float)(1.0 - h[2]);
        gs.norm = (float)norm;
        if ((int)blockIdx.x == first) {
            norms[c.group] = gs.norm;
            if (gs.skip) skipped[c.group] = skipped[c.group] + 1;
            else steps[2 * c.group] = t;
        }
    }
    __syncthreads();
    const CaGroup G = gs;
    if (G.skip && !zero) return;
    const bool vec = ca_aligned(c);
    for (int q = (int)threadIdx.x; 4 * q < c.count; q += TAP_BLOCK) {
        const int i = 4 * q;
        const bool whole = vec && i + 4 <= c.count;
        const int live = min(4, c.count - i);
        if (G.skip) {                                                      // the group's step is skipped: only g is zeroed
            if (whole) *reinterpret_cast<float4 *>(c.grad + i) = make_float4(0.f, 0.f, 0.f, 0.f);
            else
                for (int k = 0; k < live; ++k) c.grad[i + k] = 0.f;
            continue;
        }
        float p[4], g[4], m[4], v[4];
        if (whole) {
            const float4 tp = *reinterpret_cast<const float4 *>(c.param + i), tg = *reinterpret_cast<const float4 *>(c.grad + i);
            const float4 tm = *reinterpret_cast<const float4 *>(c.exp_avg + i), tv = *reinterpret_cast<const float4 *>(c.exp_avg_sq + i);
            p[0] = tp.x, p[1] = tp.y, p[2] = tp.z, p[3] = tp.w;
            g[0] = tg.x, g[1] = tg.y, g[2] = tg.z, g[3] = tg.w;
            m[0] = tm.x, m[1] = tm.y, m[2] = tm.z, m[3] = tm.w;
            v[0] = tv.x, v[1] = tv.y, v[2] = tv.z, v[3] = tv.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = k < live;
                p[k] = in ? c.param[i + k] : 0.f;
                g[k] = in ? c.grad[i + k] : 0.f;
                m[k] = in ? c.exp_avg[i + k] : 0.f;
                v[k] = in ? c.exp_avg_sq[i + k] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gc = g[k] * G.coef;
            m[k] = fmaf(G.b1, m[k], G.omb1 * gc);
            v[k] = fmaf(G.b2, v[k], G.omb2 * (gc * gc));
            const float denom = sqrtf(v[k]) / G.bc2_sqrt + G.eps;
            p[k] = p[k] - G.step_size * (m[k] / denom);
        }
        if (whole) {
            *reinterpret_cast<float4 *>(c.param + i) = make_float4(p[0], p[1], p[2], p[3]);
            *reinterpret_cast<float4 *>(c.exp_avg + i) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4 *>(c.exp_avg_sq + i) = make_float4(v[0], v[1], v[2], v[3]);
            if (zero) *reinterpret_cast<float4 *>(c.grad + i) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < live) {
                    c.param[i + k] = p[k];
                    c.exp_avg[i + k] = m[k];
                    c.exp_avg_sq[i + k] = v[k];
                    if (zero) c.grad[i + k] = 0.f;
                }
        }
    }
}


int ca_check(tap_ctx *ctx, const char *what, const void *table, int chunks, int groups, const void *ranges, const void *steps, const void *part)
{
    if (chunks < 0 || groups < 0) return tap_fail(ctx, TAP_E_INVALID, "%s: %d chunks, %d groups", what, chunks, groups);
    if (chunks == 0) return TAP_OK;
    if (groups < 1 || !table || !ranges || !steps || !part) return tap_fail(ctx, TAP_E_INVALID, "%s: null buffer or no group", what);
    if (tap_misaligned(table, 8) || tap_misaligned(ranges, 4) || tap_misaligned(steps, 8) || tap_misaligned(part, 8))
        return tap_fail(ctx, TAP_E_INVALID, "%s: the table, the counters and the partials must be 8-byte aligned", what);
    return TAP_OK;
}

} // namespace

extern "C" size_t tap_reinforce_losses_scratch(int B)
{
    if (B < 1) return 0;
    const size_t blocks = ((size_t)B + TAP_BLOCK - 1) / TAP_BLOCK;
    return 8 + blocks * 5 * sizeof(double);                                // the ticket (and its padding), then the partials
}

extern "C" int tap_reinforce_losses(tap_ctx *ctx, const float *reward, const float *critic_est, const float *tour_logp, int B, int n,
                                    float *adv_out, float *seed_logp_out, float *seed_est_out, float *stats_out, void *scratch,
                                    size_t scratch_bytes, void *stream)
{
    if (B < 0 || n < 1) return tap_fail(ctx, TAP_E_INVALID, "reinforce losses: B %d, n %d", B, n);
    if (B == 0) return TAP_OK; // an empty batch has no buffers to check
    if (!reward || !critic_est || !tour_logp || !adv_out || !seed_logp_out || !seed_est_out || !stats_out)
        return tap_fail(ctx, TAP_E_INVALID, "reinforce losses: null buffer");
    const size_t need = tap_reinforce_losses_scratch(B);
    if (!scratch || scratch_bytes < need)
        return tap_fail(ctx, TAP_E_INVALID, "reinforce losses: scratch of %zu bytes, %zu needed", scratch ? scratch_bytes : (size_t)0, need);
    const void *f32[] = {reward, critic_est, tour_logp, adv_out, seed_logp_out, seed_est_out, stats_out};
    bool bad = tap_misaligned(scratch, 8);
    for (const void *p : f32) bad = bad || tap_misaligned(p, 4);
    if (bad) return tap_fail(ctx, TAP_E_INVALID, "reinforce losses: the scratch must be 8-byte and the float buffers 4-byte aligned");
    const unsigned blocks = (unsigned)(((size_t)B + TAP_BLOCK - 1) / TAP_BLOCK);
    hipLaunchKernelGGL(k_reinforce_losses, dim3(blocks), dim3(TAP_BLOCK), 0, (hipStream_t)stream, reward, critic_est, tour_logp, B, n,
                       adv_out, seed_logp_out, seed_est_out, stats_out, reinterpret_cast<double *>(static_cast<char *>(scratch) + 8),
                       static_cast<unsigned *>(scratch));
    TAP_LAUNCH_CHECK(ctx, "k_reinforce_losses");
    return TAP_OK;
}

extern "C" int tap_clip_adam_norm(tap_ctx *ctx, const tap_adam_chunk *table, int chunks, int groups, const int32_t *ranges,
                                  int64_t *steps, double *partials, void *stream)
{
    const int rc = ca_check(ctx, "clip adam norm", table, chunks, groups, ranges, steps, partials);
    if (rc != TAP_OK || chunks == 0) return rc;
    hipLaunchKernelGGL(k_clip_adam_norm, dim3((unsigned)chunks), dim3(TAP_BLOCK), 0, (hipStream_t)stream, table, ranges, steps, partials);
    TAP_LAUNCH_CHECK(ctx, "k_clip_adam_norm");
    return TAP_OK;
}

extern "C" int tap_clip_adam_apply(tap_ctx *ctx, const tap_adam_chunk *table, int chunks, int groups, const int32_t *ranges,
                                   const double *hyper, int64_t *steps, const double *partials, float *norms_out, int32_t *skipped,
                                   int zero_grads, void *stream)
{
    const int rc = ca_check(ctx, "clip adam apply", table, chunks, groups, ranges, steps, partials);
    if (rc != TAP_OK || chunks == 0) return rc;
    if (!hyper || !norms_out || !skipped) return tap_fail(ctx, TAP_E_INVALID, "clip adam apply: null buffer");
    if (tap_misaligned(hyper, 8) || tap_misaligned(norms_out, 4) || tap_misaligned(skipped, 4))
        return tap_fail(ctx, TAP_E_INVALID, "clip adam apply: hyper must be 8-byte, norms and skipped 4-byte aligned");
    hipLaunchKernelGGL(k_clip_adam_apply, dim3((unsigned)chunks), dim3(TAP_BLOCK), 0, (hipStream_t)stream, table, ranges, hyper, steps,
                       partials, norms_out, skipped, zero_grads ? 1 : 0);
    TAP_LAUNCH_CHECK(ctx, "k_clip_adam_apply");
    return TAP_OK;
}
