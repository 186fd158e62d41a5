"""Which whole-episode (episode.hip) and rolling (rolling.hip) kernel instantiations exist in the gfx950 code objects, which
of them the API can launch (the rules restated in tests/episode_rolling_cases.py), and which the GPU cases
(episode_rolling_cases.CASES, run by tests/test_episode_rolling_variants_gpu.py) reach.  The built set is read from the
demangled `.kd` symbols of each unit's code object, taken as tests/test_store_hazards_cpu.py takes it (the library
build when fresh, else a device-only compile).  A new kernel or template argument in either file fails here until it is
restated.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

import episode_rolling_cases as S
import test_store_hazards_cpu as H
from episode_rolling_cases import (EPISODE, EPISODE_MACS2, EPISODE_MACS3, ROLL_INIT, ROLL_STEP, ROLL_WINDOW)

UNITS = ("episode", "rolling")
CXXFILT = next((p for p in (os.path.join(H.ROCM, "llvm", "bin", "llvm-cxxfilt"), shutil.which("c++filt") or "") if p and os.path.exists(p)), "c++filt")

# kernels of these units that are not instantiations of a recorded family
NOT_RECORDED = {"k_roll_zero_i32": "zeroes a roller's error flags before its first window (tap_roller_begin)"}
# built instantiations (the key without wt) the API never launches
UNREACHABLE = {}

_A = r"(-?\d+|true|false)"
_T = "<" + _A + "(?:, " + _A + ")?(?:, " + _A + ")?>"
_FAMILIES = [          # (kernel, template arguments, key without wt)
    ("k_episode", 3, lambda a: (EPISODE, a[0], a[1], a[2], 0, 0)),
    ("k_episode_macs2", 2, lambda a: (EPISODE_MACS2, 2, a[0], a[1], 0, 0)),
    ("k_episode_macs3", 2, lambda a: (EPISODE_MACS3, 3, a[0], a[1], 0, 0)),
    ("k_rolling_step", 3, lambda a: (ROLL_STEP, a[0], a[1], 0, a[2], 0)),
    ("k_rolling_step_soft", 3, lambda a: (ROLL_STEP, a[0], a[1], 1, a[2], 0)),
    ("k_rolling_window", 2, lambda a: (ROLL_WINDOW, a[0], 0, 0, a[1], 0)),
    ("k_rolling_window_wide", 2, lambda a: (ROLL_WINDOW, a[0], 0, 1, a[1], 0)),
    ("k_rolling_window_big", 2, lambda a: (ROLL_WINDOW, a[0], 0, 2, 0, a[1])),
    ("k_rolling_init", 1, lambda a: (ROLL_INIT, a[0], 0, 0, 0, 0)),
    ("k_rolling_init_big", 2, lambda a: (ROLL_INIT, a[0], 0, 1, 0, a[1])),
]


def _arg(s):
    return None if s is None else 1 if s == "true" else 0 if s == "false" else int(s)


def kernel_key(sym):
    """A demangled kernel symbol -> its launch-record key without wt, the plain name for NOT_RECORDED kernels, or an
    AssertionError for anything the restatement does not know."""
    for name, arity, key in _FAMILIES:
        m = re.match(r"^void " + name + _T + r"\(", sym)
        if m:
            a = [_arg(g) for g in m.groups() if g is not None]
            assert len(a) == arity, "template arguments of %s: %s" % (name, sym)
            return key(a)
    name = re.match(r"^(?:void )?(\w+)\(", sym)
    assert name and name.group(1) in NOT_RECORDED, "kernel not restated in tests/episode_rolling_cases.py: " + sym
    return name.group(1)


def test_kernel_key_parses_the_families():
    assert kernel_key("void k_episode<3, 16, true>(EpisodeArgs)") == (EPISODE, 3, 16, 1, 0, 0)
    assert kernel_key("void k_episode_macs3<32, 5>(EpisodeArgs)") == (EPISODE_MACS3, 3, 32, 5, 0, 0)
    assert kernel_key("void k_rolling_step_soft<2, 64, 10>(unsigned long long*, RollStepArgs)") == (ROLL_STEP, 2, 64, 1, 10, 0)
    assert kernel_key("void k_rolling_window<3, -2>(unsigned long long*, RollArgs)") == (ROLL_WINDOW, 3, 0, 0, -2, 0)
    assert kernel_key("void k_rolling_init_big<2, 64>(RollArgs)") == (ROLL_INIT, 2, 0, 1, 0, 64)
    assert kernel_key("k_roll_zero_i32(int*, int)") == "k_roll_zero_i32"
    with pytest.raises(AssertionError):
        kernel_key("void k_rolling_fancy<2>(RollArgs)")


def _symbols(unit, tmp, base, extra):
    bundle = os.path.join(tmp, unit + ".bundle")
    obj = H._fresh_build(unit)
    if obj:
        subprocess.check_call([H.OBJCOPY, "--dump-section=.hip_fatbin=" + bundle, obj, os.path.join(tmp, unit + ".host")])
    else:
        subprocess.check_call([H.HIPCC, "--offload-arch=gfx950", *base, *extra.get(unit, []), "-I" + os.path.join(H.ROOT, "include"),
                               "-I" + H.CSRC, "--cuda-device-only", "-c", os.path.join(H.CSRC, unit + ".hip"), "-o", bundle])
    co = os.path.join(tmp, unit + ".co")
    subprocess.check_call([H.BUNDLER, "--type=o", "--targets=" + H.TARGET, "--input=" + bundle, "--output=" + co, "--unbundle"])
    table = subprocess.run([H.OBJDUMP, "-t", co], check=True, capture_output=True, text=True).stdout
    mangled = sorted({line.split()[-1][:-3] for line in table.splitlines() if line.split() and line.split()[-1].endswith(".kd")})
    demangled = subprocess.run([CXXFILT], input="\n".join(mangled), check=True, capture_output=True, text=True).stdout
    return demangled.split("\n")[:len(mangled)]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    for tool in (H.HIPCC, H.BUNDLER, H.OBJDUMP, H.OBJCOPY, CXXFILT):
        if not os.path.exists(tool):
            pytest.skip("ROCm toolchain not found: " + tool)
    tmp = str(tmp_path_factory.mktemp("reach"))
    base, extra = H._make_flags()
    out = {}
    for u in UNITS:
        syms = _symbols(u, tmp, base, extra)
        assert syms, u
        out[u] = [kernel_key(s) for s in syms]
    return out


@pytest.fixture(scope="module")
def reachable():
    return S.reached(S.all_cases())


@pytest.fixture(scope="module")
def got():
    return S.reached(S.CASES)


@pytest.mark.parametrize("unit,kinds", [("episode", (EPISODE, EPISODE_MACS2, EPISODE_MACS3)),
                                        ("rolling", (ROLL_STEP, ROLL_WINDOW, ROLL_INIT))])
def test_reachable_plus_unreachable_is_built(built, reachable, unit, kinds):
    keys = {k for k in built[unit] if isinstance(k, tuple)}
    assert {k[0] for k in keys} == set(kinds)
    assert sorted(k for k in built[unit] if not isinstance(k, tuple)) == sorted(k for k in NOT_RECORDED if k.startswith("k_roll") == (unit == "rolling"))
    reached = {k[:6] for k in reachable if k[0] in kinds}
    pinned = {k for k in UNREACHABLE if k[0] in kinds}
    print("%s: %d built, %d reachable, %d unreachable" % (unit, len(keys), len(reached), len(pinned)))
    assert reached <= keys, "restated but not built: %s" % sorted(reached - keys)
    assert keys == reached | pinned, "built but neither reachable nor pinned: %s" % sorted(keys - reached - pinned)
    assert not reached & pinned, sorted(reached & pinned)


def test_built_counts(built):
    fam = lambda u, k: sum(1 for x in built[u] if isinstance(x, tuple) and x[0] == k)
    assert [fam("episode", k) for k in (EPISODE, EPISODE_MACS2, EPISODE_MACS3)] == [16, 4, 5]
    steps = [x for x in built["rolling"] if isinstance(x, tuple) and x[0] == ROLL_STEP]
    assert (sum(1 for x in steps if x[3] == 0), sum(1 for x in steps if x[3] == 1)) == (24, 16)
    assert [fam("rolling", k) for k in (ROLL_WINDOW, ROLL_INIT)] == [16, 8]


def test_cases_reach_every_reachable_key(got, reachable):
    assert got <= reachable, sorted(got - reachable)
    missing = {k[:6] for k in reachable} - {k[:6] for k in got}
    print("CASES: %d cases reach %d keys (%d without wt) of %d reachable (%d without wt)" % (
        len(S.CASES), len(got), len({k[:6] for k in got}), len(reachable), len({k[:6] for k in reachable})))
    assert not missing, sorted(missing)


def test_cases_reach_both_store_flavours(got):
    """Every rolling kind (step and window) in each D runs with write-through and with nontemporal stores."""
    for kind in (ROLL_STEP, ROLL_WINDOW):
        for D in (2, 3):
            assert {k[6] for k in got if k[0] == kind and k[1] == D} == {0, 1}, (kind, D)


def test_cases_have_unique_names_and_entries():
    names = [c.name for c in S.CASES]
    assert len(set(names)) == len(names)
    assert {c.entry for c in S.CASES} == {"reward", "scores", "pack_blocks", "rolling", "rolling_unfused", "raw_step"}
    assert {c.target for c in S.CASES if c.entry == "scores"} == {None, 0, 1}
    for c in S.CASES:
        if c.entry.startswith("rolling") or c.entry == "raw_step":
            assert 1 <= c.child <= min(c.n, 64) and c.n <= S.ROLL_MAX_N, c.name
