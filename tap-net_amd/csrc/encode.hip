// encode.hip -- the dynamic encoder on the bit shadow: the reference's first use of `dynamic` after every step is
// dynamic_hidden = self.dynamic_encoder(dynamic) (model.py:380), an nn.Conv1d(rows, hidden, kernel_size=1) over an fp32
// tensor that only ever holds 0 and 1.  A 1x1 convolution of a 0/1 tensor needs no multiplication:
//   out[b, h, c] = bias[h] + sum of W[h, r] over the rows r whose bit is set in column c's shadow word,
// added in ascending row order, one fp32 addition per row (tapenv.h: tap_encode_bits has the contract).  ONE launch turns
// the shadow (B, words) into the hidden tensor (B, H, nR); the fp32 `dynamic` is never written nor read.
//
// Forward geometry: the SPARSE form, a wavefront per (env, column) with lanes along the hidden rows.  A column's shadow
// word is then wave-uniform: the loop over its set bits is scalar (find-first-set, clear), and a lane's addend is one
// conflict-free LDS read from an [r][h] copy of the weights (row stride odd, so that the transposing fill is
// conflict-free too) -- ONE v_add per output and SET row, nothing for an unset one.  The precedence tensors are about
// 9 % ones before step 0 and only lose ones afterwards, so this is 2 .. 3 additions per output where the dense form
// (lanes along the columns, a select + add per row) pays 2.25 instructions for each of the `rows` rows; measured:
// DESIGN 7e.  Rows >= `rows` are masked off the word before the loop.  The wavefront's results go to an LDS tile
// [h][column] (row stride odd: conflict-free), and after a barrier the workgroup stores the tile as float4s, consecutive
// threads consecutive 16-byte pieces: an env's (H, nR) tile is contiguous, so with nR <= CT every wavefront store is one
// contiguous KiB (wider windows go in passes of CT columns: runs of 4 CT bytes).  A workgroup (4 wavefronts) takes a
// chunk of 128 hidden rows (two per lane) up to 64 rows, of 64 above -- weights + tile stay under 50 KB of LDS, sized
// per launch -- and a run of consecutive envs, so that the weight fill is amortised; the chunks are the grid's second
// dimension.
//
// Backward: dweight[h, r] = sum over (b, c) of g[b, h, c] * bit[b, r, c], dbias[h] = sum of g -- the same sum with a
// row of ones appended (r = rows).  Stage 1: a block takes a slice of envs and a chunk of hidden rows; per env it
// copies the chunk's g tile to LDS and TRANSPOSES the shadow by ballots into one column mask per row (which columns
// have bit r set); a thread owns up to 16 (h, r) pairs in registers and adds g & mask over the columns, in column
// order, env after env: one partial per (slice, h, r) into the caller's scratch.  Stage 2: one thread per (h, r) adds
// the slices' partials in slice order.  No atomics: two calls give the same bytes.
#include <algorithm>

#include "tap_bitshadow.h"
#include "tap_common.h"

namespace {

constexpr int TAP_HIT_ENCODE_BITS = 27; // launch record (tapenv.h: tap_variant_hits), after policy.hip's 26

__device__ __forceinline__ float enc_pick(float w, int m) { return __int_as_float(__float_as_int(w) & m); }   // w or +0.0f

struct EncArgs {
    const unsigned long long *bits; // (B, planes, nR)
    const float *weight;            // (H, rows)
    const float *bias;              // (H,) or null
    float *out;                     // (B, H, nR)
    int B, nR, rows, H, planes;
    int CT;                         // columns per pass: min(nR, 4096 / hidden rows per chunk)
    int epb;                        // consecutive envs per workgroup
};

// weights of a chunk + the output tile of a pass, in floats
inline size_t enc_lds_floats(int rows, int hck, int CT) { return (size_t)rows * (hck + 1) + (size_t)hck * (CT + 1); }

// the forward's launch: what tap_encode_bits launches with and tap_encode_bits_geometry reports
struct EncGeom {
    int planes, hpl, hck; // shadow planes; hidden rows per lane, per chunk
    int CT, epb;          // columns per pass; consecutive envs per workgroup
    int gx, gy;           // the grid: runs of envs, hidden chunks
    size_t lds;           // bytes of dynamic LDS
};
inline EncGeom enc_geom(int B, int nR, int rows, int H)
{
    EncGeom g;
    g.planes = tap_bit_planes(rows);
    g.hpl = (g.planes == 1 && H > 64) ? 2 : 1;
    g.hck = 64 * g.hpl;
    g.CT = std::min(nR, 4096 / g.hck);
    g.epb = std::max(1, B / 1024);                                         // about four workgroups per CU before a second env
    g.gx = (B + g.epb - 1) / g.epb;
    g.gy = (H + g.hck - 1) / g.hck;
    g.lds = enc_lds_floats(rows, g.hck, g.CT) * sizeof(float);            // at most 49 920 bytes
    return g;
}

template <int HPL>
__global__ void __launch_bounds__(TAP_BLOCK) k_encode_bits(EncArgs a)
{
    constexpr int HCK = 64 * HPL, S = HCK + 1;                             // hidden rows per chunk; lane l owns rows l + 64 i
    extern __shared__ float enc_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX();
    const int nR = a.nR, rows = a.rows, CT = a.CT, TS = CT + 1;
    float *lw = enc_lds, *tile = enc_lds + rows * S;
    const int hc0 = (int)blockIdx.y * HCK, hcn = min(HCK, a.H - hc0);     // this block's hidden rows hc0 .. hc0 + hcn - 1
    // W[hc0 + hl][r] -> lw[r * S + hl]: tap_fill_chunk's loop and, below, tap_rows_mask0 / 1's masks, written out: through the
    // helpers this kernel's listing changes and the launch is 2-3 % slower on the largest windows
    for (int i = tid; i < hcn * rows; i += TAP_BLOCK) {
        const int hl = i / rows, r = i - hl * rows;
        lw[r * S + hl] = a.weight[(size_t)hc0 * rows + i];
    }
    float b0[HPL];
#pragma unroll
    for (int i = 0; i < HPL; ++i) {
        const int h = hc0 + i * 64 + lane;
        b0[i] = (a.bias && h < a.H) ? a.bias[h] : 0.f;
    }
    // bits at positions >= rows are ignored: masked off each plane's word
    const unsigned long long m0 = rows >= 64 ? ~0ull : (1ull << rows) - 1;
    const unsigned long long m1 = rows >= 128 ? ~0ull : rows > 64 ? (1ull << (rows - 64)) - 1 : 0ull;
    const int e0 = (int)blockIdx.x * a.epb, e1 = min(a.B, e0 + a.epb);
    for (int env = e0; env < e1; ++env) {
        const unsigned long long *wp = a.bits + (size_t)env * (a.planes * nR);
        for (int c0 = 0; c0 < nR; c0 += CT) {
            const int ncol = min(CT, nR - c0);
            // the pass's words, one column per lane (CT <= 64); a column's word then comes by readlane: wave-uniform
            const int cc = c0 + min(lane, ncol - 1);
            const unsigned long long w0 = wp[cc] & m0, w1 = a.planes == 2 ? (wp[nR + cc] & m1) : 0ull;
            const int piece[4] = {(int)(unsigned)w0, (int)(unsigned)(w0 >> 32), (int)(unsigned)w1, (int)(unsigned)(w1 >> 32)};
            __syncthreads();                                               // the weights are in place; the tile's last stores have read it
            for (int cl = wave; cl < ncol; cl += TAP_BLOCK / 64) {
                float acc[HPL];
#pragma unroll
                for (int i = 0; i < HPL; ++i) acc[i] = b0[i];
#pragma unroll
                for (int q = 0; q < 4; ++q)                                // ascending rows: plane 0 before plane 1
                    tap_add_set_rows_piece<HPL>(lw, S, lane, q, (unsigned)__builtin_amdgcn_readlane(piece[q], cl), acc);
#pragma unroll
                for (int i = 0; i < HPL; ++i) tile[(i * 64 + lane) * TS + cl] = acc[i];
            }
            __syncthreads();
            const int q4 = ncol >> 2, total = hcn * q4;
            float *op = a.out + ((size_t)env * a.H + hc0) * nR + c0;
            for (int j = tid; j < total; j += TAP_BLOCK) {
                const int hl = j / q4, k4 = j - hl * q4;
                const float *t = tile + hl * TS + 4 * k4;
                *reinterpret_cast<float4 *>(op + (size_t)hl * nR + 4 * k4) = make_float4(t[0], t[1], t[2], t[3]);
            }
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------
constexpr int ENC_BW_PAIRS = 16;                        // (h, r) pairs a thread keeps
constexpr int ENC_BW_G_FLOATS = 8192;                   // the g tile of one env and hidden chunk in LDS (32 KB)
constexpr int ENC_BW_SLICES = 1024;                     // env slices (stage-1 partials per (h, r)), at most

struct EncBwGeom {
    int hc;      // hidden rows per chunk
    int chunks;  // ceil(H / hc)
    int slices;  // env slices
    int per;     // envs per slice
};
inline EncBwGeom enc_bw_geom(int B, int nR, int rows, int H)
{
    EncBwGeom g;
    g.hc = std::max(1, std::min(H, std::min(ENC_BW_G_FLOATS / nR, ENC_BW_PAIRS * TAP_BLOCK / (rows + 1))));
    g.chunks = (H + g.hc - 1) / g.hc;
    const int want = std::max(1, std::min(B, ENC_BW_SLICES / std::min(g.chunks, ENC_BW_SLICES)));
    g.per = (B + want - 1) / want;
    g.slices = (B + g.per - 1) / g.per;
    return g;
}

struct EncBwArgs {
    const unsigned long long *bits;
    const float *g;
    float *part;                    // (slices, H, rows + 1)
    int B, nR, rows, H, planes;
    int hc, per;
};

__global__ void __launch_bounds__(TAP_BLOCK) k_encode_bits_bw_partial(EncBwArgs a)
{
    __shared__ __attribute__((aligned(16))) float lg[ENC_BW_G_FLOATS];
    __shared__ unsigned lcm[129 * 8];                   // column masks: row r' (rows = the row of ones), 8 x 32 columns
    const int tid = threadIdx.x, lane = tid & 63, wave = TAP_WAVE_INDEX(), nR = a.nR, rows = a.rows, R1 = rows + 1;
    const int hc0 = (int)blockIdx.y * a.hc, hcn = min(a.hc, a.H - hc0), npairs = hcn * R1;
    const int e0 = (int)blockIdx.x * a.per, e1 = min(a.B, e0 + a.per);
    int goff[ENC_BW_PAIRS], moff[ENC_BW_PAIRS];
    float acc[ENC_BW_PAIRS];
#pragma unroll
    for (int i = 0; i < ENC_BW_PAIRS; ++i) {
        const int q = tid + i * TAP_BLOCK, qq = q < npairs ? q : 0, hl = qq / R1;
        goff[i] = hl * nR;
        moff[i] = (qq - hl * R1) * 8;
        acc[i] = 0.f;
    }
    const int nw = (nR + 31) >> 5;                      // 32-column mask words in use
    for (int env = e0; env < e1; ++env) {
        __syncthreads();                                // the previous env's tile has been consumed
        const float4 *src = reinterpret_cast<const float4 *>(a.g + ((size_t)env * a.H + hc0) * nR);
        for (int i = tid; i < (hcn * nR) >> 2; i += TAP_BLOCK) reinterpret_cast<float4 *>(lg)[i] = src[i];
        const unsigned long long *wp = a.bits + (size_t)env * (a.planes * nR);
        for (int base = 0; base < nR; base += 64) {     // wave-uniform loops: the ballots see every lane
            const int c = base + lane;
            const bool inr = c < nR;
            const unsigned long long w0 = inr ? wp[c] : 0ull;
            const unsigned long long w1 = (inr && a.planes == 2) ? wp[nR + c] : 0ull;
            for (int r = wave; r <= rows; r += TAP_BLOCK / 64) {
                const unsigned long long w = r < 64 ? w0 : w1;
                const bool bit = r == rows ? inr : ((w >> (r & 63)) & 1ull) != 0;
                const unsigned long long m = __ballot(bit);
                if (lane == 0) {
                    lcm[r * 8 + (base >> 5)] = (unsigned)m;
                    lcm[r * 8 + (base >> 5) + 1] = (unsigned)(m >> 32);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ENC_BW_PAIRS; ++i) {
            float s = acc[i];
            for (int cw = 0; cw < nw; ++cw) {
                const int cm = (int)lcm[moff[i] + cw], n4 = min(8, (nR - cw * 32) >> 2);
                const float4 *gp = reinterpret_cast<const float4 *>(lg + goff[i] + cw * 32);
                for (int k = 0; k < n4; ++k) {
                    const float4 v = gp[k];
                    s = s + enc_pick(v.x, __builtin_amdgcn_sbfe(cm, 4 * k, 1));
                    s = s + enc_pick(v.y, __builtin_amdgcn_sbfe(cm, 4 * k + 1, 1));
                    s = s + enc_pick(v.z, __builtin_amdgcn_sbfe(cm, 4 * k + 2, 1));
                    s = s + enc_pick(v.w, __builtin_amdgcn_sbfe(cm, 4 * k + 3, 1));
                }
            }
            acc[i] = s;
        }
    }
    float *dst = a.part + ((size_t)blockIdx.x * a.H + hc0) * R1;
#pragma unroll
    for (int i = 0; i < ENC_BW_PAIRS; ++i) {
        const int q = tid + i * TAP_BLOCK;
        if (q < npairs) dst[q] = acc[i];
    }
}

__global__ void __launch_bounds__(TAP_BLOCK) k_encode_bits_bw_reduce(const float *part, int slices, int H, int rows,
                                                                     float *dweight, float *dbias)
{
    const int R1 = rows + 1, total = H * R1, q = (int)blockIdx.x * TAP_BLOCK + (int)threadIdx.x;
    if (q >= total) return;
    float s = 0.f;
    for (int k = 0; k < slices; ++k) s = s + part[(size_t)k * total + q];   // slice order: the same bytes every call
    const int h = q / R1, r = q - h * R1;
    if (r < rows) dweight[(size_t)h * rows + r] = s;
    else if (dbias) dbias[h] = s;
}

// the checks of both entries in tap_policy_pick's order: dimensions, then the empty batch, then the caller's null check,
// then the shapes without a shadow
int enc_check_dims(tap_ctx *ctx, const char *what, int B, int nR, int rows, int H)
{
    if (B < 0 || nR < 1 || rows < 1 || H < 1) return tap_fail(ctx, TAP_E_INVALID, "%s: B %d, nR %d, rows %d, H %d", what, B, nR, rows, H);
    return TAP_OK;
}
inline bool enc_shape_ok(int nR, int rows, int H) { return tap_has_bit_shadow(rows, nR) && H <= 1024; }
int enc_check_shape(tap_ctx *ctx, const char *what, int nR, int rows, int H)
{
    if (!enc_shape_ok(nR, rows, H))
        return tap_fail(ctx, TAP_E_UNSUPPORTED, "%s: rows %d, nR %d, H %d (needs a bit shadow: rows <= 128, nR %% 4 == 0, nR <= 256; H <= 1024)",
                        what, rows, nR, H);
    return TAP_OK;
}

} // namespace

extern "C" int tap_encode_bits(tap_ctx *ctx, const unsigned long long *bits, int B, int nR, int rows, int H,
                               const float *weight, const float *bias, float *out, void *stream)
{
    int rc = enc_check_dims(ctx, "encode bits", B, nR, rows, H);
    if (rc != TAP_OK) return rc;
    if (B == 0) return TAP_OK; // an empty batch has no buffers to check
    if (!bits || !weight || !out) return tap_fail(ctx, TAP_E_INVALID, "encode bits: null buffer");
    if ((rc = enc_check_shape(ctx, "encode bits", nR, rows, H)) != TAP_OK) return rc;
    // the words are loaded one by one; out leaves as float4s
    if (tap_misaligned(bits, 8) || tap_misaligned(out, 16))
        return tap_fail(ctx, TAP_E_INVALID, "encode bits: bits must be 8-byte and out 16-byte aligned");
    const EncGeom geo = enc_geom(B, nR, rows, H);
    const EncArgs a = {bits, weight, bias, out, B, nR, rows, H, geo.planes, geo.CT, geo.epb};
    const dim3 grid((unsigned)geo.gx, (unsigned)geo.gy);
    hipStream_t st = (hipStream_t)stream;
    if (geo.hpl == 1) hipLaunchKernelGGL((k_encode_bits<1>), grid, dim3(TAP_BLOCK), geo.lds, st, a);
    else hipLaunchKernelGGL((k_encode_bits<2>), grid, dim3(TAP_BLOCK), geo.lds, st, a);
    TAP_LAUNCH_CHECK(ctx, "k_encode_bits");
    tap_variant_hit(ctx, TAP_HIT_ENCODE_BITS, 0, geo.hpl, TapVariant{geo.planes, bias ? 1 : 0, 0}, 0);
    return TAP_OK;
}

// host only: what enc_geom / enc_bw_geom give the launchers, for tests that must know which geometry a batch runs with
extern "C" int tap_encode_bits_geometry(int B, int nR, int rows, int H, int backward, int32_t out[4])
{
    if (!out) return TAP_E_INVALID;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (B < 1 || nR < 1 || rows < 1 || H < 1) return TAP_E_INVALID;
    if (!enc_shape_ok(nR, rows, H)) return TAP_E_UNSUPPORTED;
    if (backward) {
        const EncBwGeom g = enc_bw_geom(B, nR, rows, H);
        out[0] = g.per;
        out[1] = g.slices;
        out[2] = g.chunks;
        out[3] = g.hc;
    } else {
        const EncGeom g = enc_geom(B, nR, rows, H);
        out[0] = g.epb;
        out[1] = g.gx;
        out[2] = g.gy;
        out[3] = (int32_t)g.lds;
    }
    return TAP_OK;
}

extern "C" size_t tap_encode_bits_backward_scratch(int B, int nR, int rows, int H)
{
    if (B < 1 || nR < 1 || rows < 1 || H < 1 || !enc_shape_ok(nR, rows, H)) return 0;
    const EncBwGeom g = enc_bw_geom(B, nR, rows, H);
    return (size_t)g.slices * (size_t)H * (size_t)(rows + 1) * sizeof(float);
}

extern "C" int tap_encode_bits_backward(tap_ctx *ctx, const unsigned long long *bits, const float *g, int B, int nR, int rows,
                                        int H, float *dweight, float *dbias, void *scratch, size_t scratch_bytes, void *stream)
{
    int rc = enc_check_dims(ctx, "encode bits backward", B, nR, rows, H);
    if (rc != TAP_OK) return rc;
    if (B == 0) return TAP_OK; // (an empty batch leaves dweight / dbias as they are)
    if (!bits || !g || !dweight) return tap_fail(ctx, TAP_E_INVALID, "encode bits backward: null buffer");
    if ((rc = enc_check_shape(ctx, "encode bits backward", nR, rows, H)) != TAP_OK) return rc;
    const size_t need = tap_encode_bits_backward_scratch(B, nR, rows, H);
    if (!scratch || scratch_bytes < need)
        return tap_fail(ctx, TAP_E_INVALID, "encode bits backward: scratch of %zu bytes, %zu needed", scratch ? scratch_bytes : (size_t)0, need);
    // g is copied to LDS as float4s; the words and the partials go one by one
    if (tap_misaligned(bits, 8) || tap_misaligned(g, 16) || tap_misaligned(scratch, 4))
        return tap_fail(ctx, TAP_E_INVALID, "encode bits backward: bits must be 8-byte, g 16-byte and scratch 4-byte aligned");
    const EncBwGeom geo = enc_bw_geom(B, nR, rows, H);
    const EncBwArgs a = {bits, g, static_cast<float *>(scratch), B, nR, rows, H, tap_bit_planes(rows), geo.hc, geo.per};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_encode_bits_bw_partial, dim3((unsigned)geo.slices, (unsigned)geo.chunks), dim3(TAP_BLOCK), 0, st, a);
    TAP_LAUNCH_CHECK(ctx, "k_encode_bits_bw_partial");
    const int total = H * (rows + 1);
    hipLaunchKernelGGL(k_encode_bits_bw_reduce, dim3((unsigned)((total + TAP_BLOCK - 1) / TAP_BLOCK)), dim3(TAP_BLOCK), 0, st,
                       static_cast<const float *>(scratch), geo.slices, H, rows, dweight, dbias);
    TAP_LAUNCH_CHECK(ctx, "k_encode_bits_bw_reduce");
    tap_variant_hit(ctx, TAP_HIT_ENCODE_BITS, 0, 0, TapVariant{a.planes, dbias ? 1 : 0, 1}, 0);
    return TAP_OK;
}
