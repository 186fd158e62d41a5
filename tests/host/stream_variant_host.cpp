// Host build of tap-net_amd/csrc/tap_stream_variant.h (the choice of a stream-wave kernel's instantiation and each
// launcher's table of instantiations) behind C entry points, for tests/test_stream_variant_cpu.py.
#include <cstddef>

#include "tap_stream_variant.h"

// built with -fvisibility=hidden: the tables are inline variables, which would otherwise bind to the first of the test's
// A/B builds loaded into the process
#define SV_API extern "C" __attribute__((visibility("default")))

namespace {

template <int KIND> constexpr int table_size() { return (int)(sizeof(TapVariants<KIND>::v) / sizeof(TapVariant)); }

template <int KIND> bool table_entry(int i, int *out)
{
    if (i < 0 || i >= table_size<KIND>()) return false;
    const TapVariant &e = TapVariants<KIND>::v[i];
    out[0] = e.nc; out[1] = e.mode; out[2] = e.extra;
    return true;
}

}   // namespace

// row i of f (16 ints): nc, src, inplace, inputs, wt, n, rows, update_rows, nR, D, G, EPB, B, W, L, hard;
// row i of out (3 ints): nc, mode, extra
SV_API void sv_select(int kind, int rows, const int *f, int *out)
{
    for (int i = 0; i < rows; ++i, f += 16, out += 3) {
        const TapMaskFacts m{f[0], f[1], f[2] != 0, f[3] != 0, f[4] != 0, f[5], f[6], f[7], f[8]};
        const TapLaunchFacts l{f[9], f[10], f[11], f[12], f[13], f[14], f[15] != 0};
        const TapVariant v = tap_stream_variant(kind, m, l);
        out[0] = v.nc; out[1] = v.mode; out[2] = v.extra;
    }
}

SV_API int sv_kinds() { return TAP_SV_KINDS; }

// entry i of launcher kind's table -> 1, 0 past its end
SV_API int sv_table_entry(int kind, int i, int *out)
{
    switch (kind) {
    case TAP_SV_TRANSITION: return table_entry<TAP_SV_TRANSITION>(i, out);
    case TAP_SV_MACS: return table_entry<TAP_SV_MACS>(i, out);
    case TAP_SV_MACS3: return table_entry<TAP_SV_MACS3>(i, out);
    case TAP_SV_BIG: return table_entry<TAP_SV_BIG>(i, out);
    case TAP_SV_MACS_WAVE: return table_entry<TAP_SV_MACS_WAVE>(i, out);
    case TAP_SV_MACS3_WAVE: return table_entry<TAP_SV_MACS3_WAVE>(i, out);
    case TAP_SV_MASK_STEP: return table_entry<TAP_SV_MASK_STEP>(i, out);
    default: return 0;
    }
}

SV_API int sv_built(int kind, int D, int G, int nc, int mode, int extra)
{
    return tap_variant_built(kind, D, G, TapVariant{nc, mode, extra});
}
