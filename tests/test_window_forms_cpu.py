"""The window forms of tests/window_forms.py on the CPU: tests/golden/window_forms.npz (the reference's pack.update_dynamic /
pack.update_mask / pack.reward and the mask of model.py:297-307 on R = 1, 'rot-old', 'bot'/False, the 3n-row input types and
'mul-with') pins the oracle bit for bit; the case table covers what tests/test_window_forms_gpu.py is meant to run; the
inputs of every GPU case are usable (a first mask with both values, no block that fails to fit); the host build of the
kernel selector gives no neighbour of a compiled-in window its bits."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
import oracle_lib as O
import ref_loader
import stream_cases as S
import window_forms as WF

SEEDS = (0, 1)                 # the instance seeds the GPU file uses (one per episode of a stepper path)


def _digest(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a, dtype=np.float32).tobytes(), digest_size=8).digest(), np.uint8)


@pytest.fixture(scope="module")
def rec():
    return G.load("window_forms.npz")


def test_fixture_lists_the_table(rec):
    assert [k.decode() for k in rec["cases"]] == [c.name for c in WF.GOLDEN_CASES]
    assert [k.decode() for k in rec["tours"]] == [WF.tour_key(f, s, D, W) for f, s in WF.TOURS for D, W in WF.TOUR_CONTAINERS]
    assert os.path.getsize(os.path.join(G.GOLDEN, "window_forms.npz")) < os.path.getsize(os.path.join(G.GOLDEN, "masks_2d.npz")) // 2


@pytest.mark.parametrize("case", WF.GOLDEN_CASES, ids=lambda c: c.name)
def test_oracle_equals_the_reference(rec, case):
    """update_dynamic, both masks of update_mask and the initial mask, after every step of the case's tape"""
    k = [v.decode() for v in rec["cases"]].index(case.name)
    want = rec["digests"][rec["offsets"][k]:rec["offsets"][k + 1]]
    assert want.shape == (1 + 3 * case.nsteps, 8)
    run = WF.oracle_run(O, case, WF.build(case, seed=0), placement=False)
    assert np.array_equal(_digest(run["initial"]), want[0]), "initial mask"
    for t in range(case.nsteps):
        for j, what in enumerate(("dynamic", "current", "mask")):
            assert np.array_equal(_digest(run[what][t]), want[1 + 3 * t + j]), "%s after step %d" % (what, t)


def _oracle_tour_ratio(c, static, tour):
    """What pack.reward's calc_positions_* calls return (pack.py:438-471) -> (B, 2) float64"""
    fn = O.calc_positions_mcs if c.strategy == "MACS" else O.calc_positions_lb_greedy
    out = np.zeros((c.B, 2), np.float64)
    for b in range(c.B):
        sample = static[b][:, tour[b][:c.n]]
        blocks = sample[1:1 + c.D].T.astype(np.int32)
        lists = [blocks[sample[-1] == t] for t in (0, 1)] if c.input_type == "mul-with" else [blocks]
        for j, mine in enumerate(lists):
            if len(mine):
                rc, _, _, out[b, j], _ = fn(mine, list(c.cs), c.reward)
                assert rc == 0
    return out


@pytest.mark.parametrize("tour", [(f, s, D, W) for f, s in WF.TOURS for D, W in WF.TOUR_CONTAINERS],
                         ids=lambda t: WF.tour_key(*t))
def test_oracle_reward_equals_the_reference(rec, tour):
    c = WF.tour_case(*tour)
    k = [v.decode() for v in rec["tours"]].index(WF.tour_key(*tour))
    static, tp = WF.tour_inputs(c)
    got = _oracle_tour_ratio(c, static, tp)
    want = rec["tour_ratio"][k]
    assert got.dtype == want.dtype == np.float64
    assert (got == want).all(), (got, want)
    # pack.py:448, 469-473: the scores tensor is float32; 'mul-with' stores the mean of the two lists
    score = (got[:, 0] + got[:, 1]) / 2 if c.input_type == "mul-with" else got[:, 0]
    assert np.array_equal(-score.astype(np.float32), rec["tour_reward"][k])


def test_generator_reproduces_the_fixture(tmp_path):
    if not ref_loader.available():
        pytest.skip("the reference checkout is not present")
    out = str(tmp_path / "window_forms.npz")
    subprocess.check_call([sys.executable, os.path.join(G.GOLDEN, "make_golden_window_forms.py"), out])
    with open(out, "rb") as a, open(os.path.join(G.GOLDEN, "window_forms.npz"), "rb") as b:
        assert a.read() == b.read()


# ---- the table -------------------------------------------------------------------------------------------------------
def test_forms_are_the_reference_s():
    """rows, update_rows, R and static rows of every form, against pack.py:276-376 restated per input type"""
    want = {"simple": (1, 0, 1, 1, 0), "rot1": (1, 0, 1, 1, 0), "rot-old": (1, 1, 1, None, 0), "rot-old1": (1, 1, 1, 1, 0),
            "bot1": (3, 0, 3, 1, 0), "bot-rot": (3, 0, 3, None, 0), "use-static": (3, 0, 3, None, 0),
            "use-pnet": (3, 0, 3, None, 0), "mul-with": (3, 0, 3, None, 1), "bot": (3, 0, 3, None, 0)}
    assert set(want) == set(WF.FORMS)
    for form, (a, b, ur, R, extra) in want.items():
        for D in (2, 3):
            c = WF.Case(form, D, WF.LB2 if D == 2 else WF.LB3, 7)
            assert (c.rows, c.update_rows, c.R, c.static_rows) == (7 * a + b, ur, R or (2 if D == 2 else 6), 1 + D + extra)


def test_every_form_runs_every_path():
    pairs = {(c.form, p) for c in WF.CASES for p in c.paths}
    for form in WF.FORMS:
        for p in WF.PATHS:
            assert (form, p) in pairs, "no case runs form %r on path %r" % (form, p)
    assert {f for f, p in pairs if p == "rollout"} == set(WF.ROLLOUT_FORMS)
    assert {f for f, _ in WF.TOURS} >= {"simple", "rot-old", "mul-with"} and {s for _, s in WF.TOURS} == {"LB_GREEDY", "MACS"}


def test_every_shape_is_in_the_table():
    for form, D, n in WF.REQUIRED_SHAPES:
        hits = [c for c in WF.CASES if (c.form, c.D, c.n, c.cs) == (form, D, n, WF.LB2 if D == 2 else WF.LB3)
                and c.strategy == "LB_GREEDY"]
        assert {c.B for c in hits} == {64, 67}, (form, D, n)
        for c in hits:
            assert "seams" in c.paths and "stepper" in c.paths
    for strategy, cs in WF.REQUIRED_FAMILIES:
        hits = [c for c in WF.CASES if c.strategy == strategy and c.cs == cs]
        assert any(c.form == "rot-old" for c in hits) and any(c.R == 1 for c in hits), (strategy, cs)
        for c in hits:
            assert "seams" in c.paths and "stepper" in c.paths and "env_transition" in c.paths
            assert not (c.strategy == "MACS" and c.D == 3 and c.cells <= 8)
    assert len({c.name for c in WF.CASES}) == len(WF.CASES)
    for c in WF.CASES:
        assert c.nsteps == (c.n if c.n <= 20 else 4) and c.cs[-1] >= 4 * c.nsteps


def test_the_edges_the_shapes_were_chosen_for():
    by = {(c.form, c.D, c.n, c.strategy, c.cs): c for c in WF.CASES}
    g = lambda form, D, n, strategy="LB_GREEDY", cs=None: by[(form, D, n, strategy, cs or (WF.LB2 if D == 2 else WF.LB3))]  # noqa: E731
    assert not S.shadow_ok(g("simple", 2, 10)) and S._copy_cols(g("simple", 2, 10)) == 0
    assert S.shadow_ok(g("simple", 2, 12)) and S._cols(12) == 1
    c = g("bot1", 2, 20)
    assert (c.nR, c.rows) == (20, 60) and S.shadow_ok(c)
    assert (g("simple", 2, 64).rows, g("simple", 2, 64).nR) == (64, 64) and WF.predicted_kind(g("simple", 2, 64)) == S.TRANSITION
    c = g("simple", 2, 68)
    assert S.shadow_ok(c) and S._cols(c.nR) == 2 and WF.predicted_kind(c) == S.MASK_STEP
    assert (g("rot-old", 2, 10).nR, g("rot-old", 2, 10).rows) == (20, 11)
    assert (g("rot-old", 3, 10).nR, g("rot-old", 3, 10).rows) == (60, 11)
    assert g("rot-old", 2, 32).rows == 33 and S.shadow_ok(g("rot-old", 2, 32))
    assert g("rot-old", 2, 31).rows == 32 and g("rot-old", 2, 63).rows == 64
    c = g("rot-old", 2, 64)
    assert c.rows == 65 and S.shadow_ok(c) and WF.predicted_kind(c) == S.MASK_STEP
    assert not S.shadow_ok(g("rot-old", 2, 9))
    c = g("rot-old", 2, 20, "MACS", (7, 200))
    assert (c.nR, c.rows) == (40, 21) and WF.predicted_kind(c) == S.MACS
    assert g("simple", 2, 40, "MACS", (7, 200)).nR == 40
    assert WF.predicted_kind(g("rot-old", 3, 10, "MACS")) == S.MACS3
    assert WF.predicted_kind(g("rot-old", 3, 10, cs=(10, 10, 200))) == S.BIG
    assert WF.predicted_kind(g("rot-old", 2, 10, "MACS", (20, 200))) == S.MACS_WAVE
    assert WF.predicted_kind(g("rot-old", 3, 10, "MACS", (9, 9, 200))) == S.MACS3_WAVE


# ---- the inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WF.CASES, ids=lambda c: c.name)
def test_inputs_are_usable(case):
    """the first current_mask holds both 0 and 1 and the oracle raises no error bit over the whole case; row 0 of static
    is not `column mod n`, and the tape's cleared rows differ from the dropped columns"""
    for seed in SEEDS:
        inp = WF.build(case, seed)
        run = WF.oracle_run(O, case, inp)
        first = run["initial"]
        assert (first == 0).any() and (first == 1).any(), seed
        assert run["episode"]["nerr"] == 0 and not run["episode"]["errs"].any(), seed
        st0, tape = inp["static"][:, 0, :], inp["tape"]
        assert st0.min() == 0 and st0.max() == case.n - 1
        for r in range(case.R):
            assert (np.sort(st0[:, r * case.n:(r + 1) * case.n], 1) == np.arange(case.n)).all()
        real = np.take_along_axis(st0, tape, 1)
        if case.n > 2:
            assert (real != tape % case.n).any()
        nodes = np.sort(tape % case.n, 1)
        assert (nodes[:, 1:] != nodes[:, :-1]).all() and 0 <= tape.min() and tape.max() < case.nR     # a permutation per env
        assert len({tuple(row) for row in tape.tolist()}) > 1
        nb = WF.build(case, seed, nonbinary=True)["dynamic"]
        assert 3 <= ((nb != 0) & (nb != 1)).sum() <= 7 and (nb != inp["dynamic"]).sum() <= 7


# ---- the selector ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sv():
    lib = S.selector()
    if lib is None:
        pytest.skip("no g++ for the host build of the selector")
    return lib


def _stepper_keys(sv, c):
    from dataclasses import replace
    out = set()
    for path in ("stepper",) + (WF.SHADOW_PATHS if S.shadow_ok(c) else ()):
        for init in (True, False):
            out |= S.keys(sv, S.launches(replace(c, path=path, init_mask=init)))
    return out


@pytest.mark.parametrize("case", WF.CASES, ids=lambda c: c.name)
def test_selector_keeps_the_forms_off_the_compiled_in_windows(sv, case):
    WF.check_keys(case, _stepper_keys(sv, case))


COMPILED_IN = [  # (kind, launch facts, the window's four shape facts): c2's, c3's (k_transition), c4's (k_transition_macs)
    (S.TRANSITION, dict(D=2, G=8, EPB=8, B=64, W=0, L=0, hard=0), dict(n=10, rows=30, update_rows=3, nR=20)),
    (S.TRANSITION, dict(D=3, G=32, EPB=8, B=64, W=0, L=0, hard=0), dict(n=10, rows=30, update_rows=3, nR=60)),
    (S.MACS, dict(D=2, G=8, EPB=8, B=64, W=7, L=1, hard=0), dict(n=20, rows=60, update_rows=3, nR=40)),
]


@pytest.mark.parametrize("window", range(len(COMPILED_IN)))
def test_selector_refuses_every_neighbour_of_a_compiled_in_window(sv, window):
    """n, rows, update_rows and nR reach the kernels as independent run-time values (the C ABI takes each): a window that
    differs from a compiled-in one in ANY one of them -- the values the forms here give it: 'rot-old' rows = n + 1 and
    update_rows = 1, R = 1 columns -- must run the run-time-shaped kernel."""
    kind, lf, shape = COMPILED_IN[window]
    base = dict(nc=1, src=1, inplace=0, inputs=1, wt=1, **shape, **lf)
    (nc, mode, extra), = S.select(sv, kind, [base])
    assert mode & 24 != 0 and (kind != S.MACS or extra == 7)         # the window itself is compiled in
    n = shape["n"]
    others = dict(n=[n + 1, n // 2, 2 * n], rows=[n + 1, n, 3 * n - 1, 3 * n + 1, 2 * n], update_rows=[1, 0, 2],
                  nR=[shape["nR"] // 2, shape["nR"] + 4, 4 * n])
    for fact, values in others.items():
        for v in values:
            if v == shape[fact]:
                continue
            for src in (1, 2):
                (nc, mode, extra), = S.select(sv, kind, [dict(base, src=src, **{fact: v})])
                assert mode & (24 | 64) == 0 and extra == 0, "%s = %d still selects mode %d extra %d" % (fact, v, mode, extra)
