"""Which precedence-update ("stream wave") kernel instantiations the API can launch, and which of them the GPU cases
(tests/stream_cases.CASES, run by tests/test_stream_variants_gpu.py) reach, for all seven launchers.  The launcher rules
are restated in tests/stream_cases.py; the answer for each launch comes from the host build of tap_stream_variant.h.
No GPU needed."""
import pytest

import stream_cases as S
from stream_cases import MACS, MACS3, MACS_WAVE, MASK_STEP, TRANSITION

KINDS = range(7)
DG = {TRANSITION: [(D, G) for D in (2, 3) for G in (8, 16, 32, 64)], MACS: [(2, 8), (2, 16)],
      MACS3: [(3, G) for G in (8, 16, 32, 64)]}

# Built entries (kind, D, G, nc, mode, extra) the API never launches.  All are 2D windows on the bit shadow with nc = 4:
# the one-launch steps carry rows <= 64 (tap_step_request.h: tap_step_route), so 'bot' has n <= 21 (nR <= 42) and 'rot' n <= 64
# (nR <= 128), which gives nc <= 2.  The fp32-copy entries {4, 0} ARE reachable: 'bot' n = 65 .. 128 is the stepper's
# copy form (rows > 128) with nR = 130 .. 256, and tap_transition takes any window.
_BITS = "2D step on the bit shadow: rows <= 64 bounds nR by 128"
UNREACHABLE = {
    **{(TRANSITION, 2, G, 4, m, 0): _BITS for G in (8, 16, 32, 64) for m in (1 | 32, 5, 1, 6, 2)},
    **{(MACS, 2, G, 4, m, 0): _BITS for G in (8, 16) for m in (1 | 32, S.TAP_MACS_M1, S.TAP_MACS_M2)},
    **{(MACS_WAVE, 0, 0, 4, m, 0): _BITS + " (the MACS 2D wave kernel is 2D only)" for m in (1, 2)},
}


@pytest.fixture(scope="module")
def sv():
    lib = S.selector()
    if lib is None:
        pytest.skip("no g++")
    return lib


@pytest.fixture(scope="module")
def reachable(sv):
    return S.reached(sv, S.all_cases(), steps=2)


@pytest.fixture(scope="module")
def got(sv):
    return S.reached(sv, S.CASES)


def _built(lib, kind):
    return {(kind, D, G) + v for D, G in DG.get(kind, [(0, 0)]) for v in S.table(lib, kind) if lib.sv_built(kind, D, G, *v)}


@pytest.mark.parametrize("kind", KINDS)
def test_reachable_plus_unreachable_is_built(sv, reachable, kind):
    built = _built(sv, kind)
    reached = {k[:6] for k in reachable if k[0] == kind}
    assert reached <= built, sorted(reached - built)
    pinned = {k for k in UNREACHABLE if k[0] == kind}
    assert built - reached == pinned, "unreachable but not pinned: %s; pinned but reachable: %s" % (
        sorted(built - reached - pinned), sorted(pinned - (built - reached)))


def test_built_counts(sv):
    assert [len(_built(sv, k)) for k in KINDS] == [180, 29, 65, 12, 6, 6, 16]


def test_cases_reach_every_reachable_entry(got, reachable):
    assert got <= reachable, sorted(got - reachable)
    assert {k[:6] for k in got} == {k[:6] for k in reachable}, sorted({k[:6] for k in reachable} - {k[:6] for k in got})


def test_cases_reach_both_store_flavours(got, reachable):
    """Every entry reachable with write-through stores is reached with them (every entry of these launchers can expand
    the fp32 tensor); every (launcher, nc) reachable with nontemporal stores is run with them at least once."""
    wt1 = {k[:6] for k in reachable if k[6] == 1}
    assert wt1 <= {k[:6] for k in got if k[6] == 1}, sorted(wt1 - {k[:6] for k in got if k[6] == 1})
    wt0 = {(k[0], k[3]) for k in reachable if k[6] == 0}
    assert wt0 <= {(k[0], k[3]) for k in got if k[6] == 0}, sorted(wt0 - {(k[0], k[3]) for k in got if k[6] == 0})


def test_cases_have_runners_and_unique_names():
    names = [c.name for c in S.CASES]
    assert len(set(names)) == len(names)
    paths = {"stepper", "inplace", "noexpand", "seam_bits", "seam_mask_step", "seam_transition", "seam_transition_bits"}
    assert {c.path for c in S.CASES} <= paths
    assert all(c.offset % 16 == 0 and (c.offset == 0 or c.path.startswith("seam")) for c in S.CASES)
