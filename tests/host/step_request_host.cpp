// Host build of tap-net_amd/csrc/tap_step_request.h -- the shadow predicate, the request check and the route of a fused
// step -- behind C entry points, for tests/test_step_request_cpu.py.  With -DSTEP_REQUEST_HOST_MAIN the file is a
// stand-alone program that sweeps the route and the check against a restatement (the form that is run under sanitizers).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "tap_step_request.h"

extern "C" int srq_has_shadow(int rows, int nR) { return tap_window_has_shadow(rows, nR) ? 1 : 0; }

static tap_env_desc desc_of(int strategy, int D, int W, int L)
{
    tap_env_desc d = {};
    d.strategy = strategy; d.D = D; d.W = W; d.L = L;
    return d;
}

// caps: bit 0 big_ok, 1 macs_wave_ok, 2 macs3_wave_ok, 3 macs_lanes_fit; -> TapStepRoute
extern "C" int srq_route(int form, int rows, int strategy, int D, int W, int L, int caps, int macs2d_wave_from)
{
    TapStepRequest r = {};
    r.form = form; r.rows = rows;
    const TapStepCaps c = {(caps & 1) != 0, (caps & 2) != 0, (caps & 4) != 0, (caps & 8) != 0, macs2d_wave_from};
    return tap_step_route(r, desc_of(strategy, D, W, L), c);
}

extern "C" int srq_route_launches(int route) { return tap_step_route_launches((TapStepRoute)route); }

// ints: n, R, rows, update_rows, static_rows, flags; ptrs: 14 values taken as addresses, in TapStepRequest's order (dyn_in,
// bits_in, static, ptr, mask_in, colsum_in, dyn_out, colsum_out, bits_out, current_out, mask_out, feature_out, ratio_out,
// nonbinary_out); nothing is dereferenced.  -> status; msg (64 bytes) takes the message
extern "C" int srq_check(int form, const int *ints, const uintptr_t *ptrs, int B, int D, int from_stepper, int has_state, char *msg)
{
    TapStepRequest r = {};
    r.form = form;
    r.n = ints[0]; r.R = ints[1]; r.rows = ints[2]; r.update_rows = ints[3]; r.static_rows = ints[4]; r.flags = ints[5];
    r.dyn_in = (const float *)ptrs[0]; r.bits_in = (const unsigned long long *)ptrs[1]; r.static_ = (const float *)ptrs[2];
    r.ptr = (const int64_t *)ptrs[3]; r.mask_in = (const float *)ptrs[4]; r.colsum_in = (const float *)ptrs[5];
    r.dyn_out = (float *)ptrs[6]; r.colsum_out = (float *)ptrs[7]; r.bits_out = (unsigned long long *)ptrs[8];
    r.current_out = (float *)ptrs[9]; r.mask_out = (float *)ptrs[10]; r.feature_out = (float *)ptrs[11];
    r.ratio_out = (float *)ptrs[12]; r.nonbinary_out = (int32_t *)ptrs[13];
    const TapStepVerdict v = tap_step_request_check(r, B, D, from_stepper != 0, has_state != 0);
    if (msg) snprintf(msg, 64, "%s", v.msg ? v.msg : "");
    return v.status;
}

#ifdef STEP_REQUEST_HOST_MAIN
// the routing as transition.hip had it before the header: the wave kind first, then the lane kernels, then two launches
static int old_route(int form, int rows, const tap_env_desc &d, int caps, int from)
{
    const bool big = d.strategy == TAP_LB_GREEDY && (d.W * d.L > 64 || (d.D == 3 && (d.W > 8 || d.L > 8)));
    const bool big3 = d.strategy == TAP_MACS && d.D == 3 && (d.W * d.L > 64 || d.W > 8 || d.L > 8);
    int kind = 0;
    if (rows > 64) kind = 0;
    else if (big) kind = (caps & 1) ? 1 : 0;
    else if (d.strategy != TAP_MACS) kind = 0;
    else if (d.D == 2) kind = (d.W > 16 && d.W >= from && (caps & 2)) ? 2 : 0;
    else kind = (big3 && (caps & 4)) ? 3 : 0;
    bool single = !(d.strategy == TAP_LB || big || big3 || (d.strategy == TAP_MACS && d.D == 2 && d.W > 16));
    if (single && d.strategy == TAP_MACS && !(caps & 8)) single = false;
    if (form != TAP_STEP_COPY && kind) return kind;
    return (single && (form == TAP_STEP_COPY || rows <= 64)) ? 0 : 4;
}

int main()
{
    long checked = 0;
    for (int strategy : {TAP_LB_GREEDY, TAP_MACS, TAP_LB})
        for (int D = 2; D <= 3; ++D)
            for (int W = 1; W <= 70; W += (W < 20 ? 1 : 7))
                for (int L = 1; L <= (D == 3 ? 12 : 1); ++L)
                    for (int form = 0; form < 3; ++form)
                        for (int rows : {1, 63, 64, 65, 128, 129})
                            for (int caps = 0; caps < 16; ++caps)
                                for (int from : {17, 33}) {
                                    const int got = srq_route(form, rows, strategy, D, W, L, caps, from);
                                    const int want = old_route(form, rows, desc_of(strategy, D, W, L), caps, from);
                                    ++checked;
                                    if (got != want || srq_route_launches(got) != (want == 4 ? 2 : 1)) {
                                        printf("route: strategy %d D %d %dx%d form %d rows %d caps %d from %d: %d, want %d\n", strategy, D, W, L,
                                               form, rows, caps, from, got, want);
                                        return 1;
                                    }
                                }
    // the check: every subset of null pointers on a valid window, against the lists transition.hip had
    const int ints[6] = {4, 2, 12, 3, 3, TAP_T_RATIO};
    char msg[64];
    for (int form = 0; form < 3; ++form)
        for (unsigned nulls = 0; nulls < (1u << 14); ++nulls)
            for (int stepper = 0; stepper < 2; ++stepper) {
                uintptr_t p[14];
                for (int i = 0; i < 14; ++i) p[i] = (nulls >> i & 1) ? 0 : 0x1000 + 0x100 * (uintptr_t)i;
                const bool common = !p[2] || !p[3] || (!p[4] && !stepper) || !p[9] || !p[10] || !p[12];
                const bool own = form == TAP_STEP_COPY ? (!p[0] || !p[5] || !p[6] || !p[7]) : form == TAP_STEP_BITS ? (!p[1] || !p[8]) : (!p[0] || !p[8]);
                const char *want = common ? "bad transition arguments" : !own ? "" : form == TAP_STEP_COPY ? "bad transition arguments"
                                   : form == TAP_STEP_BITS ? "bad transition_bits arguments" : "bad transition_first arguments";
                const int rc = srq_check(form, ints, p, 8, 2, stepper, 1, msg);
                ++checked;
                if (rc != (*want ? TAP_E_INVALID : TAP_OK) || strcmp(msg, want) != 0) {
                    printf("check: form %d nulls %x stepper %d: %d '%s', want '%s'\n", form, nulls, stepper, rc, msg, want);
                    return 1;
                }
                if (srq_check(form, ints, p, 0, 2, stepper, 0, msg) != TAP_OK) { printf("check: B = 0 refused\n"); return 1; }
            }
    for (int rows = 1; rows <= 130; ++rows)
        for (int nR = 1; nR <= 262; ++nR, ++checked)
            if (srq_has_shadow(rows, nR) != (rows <= 128 && nR % 4 == 0 && nR <= 256)) { printf("shadow %d %d\n", rows, nR); return 1; }
    printf("step request host: %ld values ok\n", checked);
    return 0;
}
#endif
