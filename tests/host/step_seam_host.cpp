// Host build of the host-compilable part of tap-net_amd/csrc/tap_step_seam.h -- the strided feature writer and the
// admission function -- behind C entry points, for tests/test_step_seam_host_cpu.py.  With -DSEAM_HOST_MAIN the file is a
// stand-alone program that runs both over a sweep of shapes (the form that is run under sanitizers).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tap_step_seam.h"

// what the unit's member `first` of `stride` writes; zero_min: the minimum over the whole map (what the unit's reduction
// returns to every member)
extern "C" void seam_feature(int feature, int D, int W, int L, const int32_t *hm, float *out, int first, int stride, int zero_min)
{
    tap_seam_feature(feature, D, W, L, hm, out, first, stride, [zero_min](int) { return zero_min; });
}

// -> do_step; *err = the error bits raised
extern "C" int seam_admit(int act, int count, int n_max, int bx, int by, int bz, int family_rejects, int *err)
{
    int e = 0;
    const bool go = tap_seam_admit(act != 0, count, n_max, bx, by, bz, family_rejects != 0, e);
    *err = e;
    return go ? 1 : 0;
}

#ifdef SEAM_HOST_MAIN
int main()
{
    long checked = 0;
    for (int D = 2; D <= 3; ++D)
        for (int W = 1; W <= 70; W += 3)
            for (int L = 1; L <= (D == 3 ? 13 : 1); L += 4) {
                const int cells = W * L;
                std::vector<int32_t> hm(cells);
                int mn = INT_MAX;
                for (int c = 0; c < cells; ++c) { hm[c] = (c * 7919 + W) % 23; mn = hm[c] < mn ? hm[c] : mn; }
                for (int feature = 0; feature < 3; ++feature) {
                    const int flen = feature == TAP_FEAT_DIFF ? (D == 2 ? W - 1 : 2 * cells) : cells;
                    std::vector<float> ref(flen > 0 ? flen : 1, -1.f);
                    seam_feature(feature, D, W, L, hm.data(), ref.data(), 0, 1, mn);
                    for (int stride : {64, 256}) {
                        std::vector<float> out(flen > 0 ? flen : 1, -1.f);
                        for (int first = 0; first < stride; ++first) seam_feature(feature, D, W, L, hm.data(), out.data(), first, stride, mn);
                        for (int k = 0; k < flen; ++k, ++checked)
                            if (out[k] != ref[k]) { printf("feature %d D %d %dx%d stride %d: out[%d]\n", feature, D, W, L, stride, k); return 1; }
                    }
                }
            }
    for (int act = 0; act < 2; ++act)
        for (int count = 0; count < 3; ++count)
            for (int side = 0; side < 3; ++side)
                for (int fam = 0; fam < 2; ++fam, ++checked) {
                    int err;
                    const int go = seam_admit(act, count, 2, side, 1, 1, fam, &err);
                    const int want = act ? ((count >= 2 ? 2 : 0) | ((side < 1 || fam) ? 4 : 0)) : 0;
                    if (err != want || go != (act && !want)) { printf("admit %d %d %d %d\n", act, count, side, fam); return 1; }
                }
    printf("step seam host: %ld values ok\n", checked);
    return 0;
}
#endif
