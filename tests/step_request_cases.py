"""What the fused step's entry points refuse before any launch: one table for the host build of tap_step_request.h
(tests/test_step_request_cpu.py: tap_step_request_check) and for the C ABI on the GPU (tests/test_step_request_gpu.py).

A row starts from a valid request of its form on the smallest window with a bit shadow -- 2D, n = 4, R = 2 (nR = 8), rows =
12, update_rows = 3, static_rows = 1 + D = 3, every pointer its form uses given -- and breaks one thing.  Each row was read
off the checks of transition.hip (transition_impl, which runs tap_step_request_check; tap_transition's own mask_in test)
and masks.hip (tap_mask_step_bits / _first).  `mask_step` says whether the stand-alone tap_mask_step_bits / _first of the
row's form refuses the same arguments too; where it would launch (it needs fewer buffers: no mask_in, one output of four,
static_rows >= 1) the row is not handed to it."""
from dataclasses import dataclass

COPY, BITS, FIRST = 0, 1, 2                      # tap_step_request.h: TapStepForm
FORM_NAMES = {COPY: "copy", BITS: "bits", FIRST: "first"}
TAP_OK, TAP_E_INVALID, TAP_E_UNSUPPORTED = 0, -1, -2
TAP_T_FRESH, TAP_T_RATIO = 1, 2
D, N, R, ROWS, UPDATE_ROWS, STATIC_ROWS = 2, 4, 2, 12, 3, 3

# TapStepRequest's pointer fields, in its order
POINTERS = ["dyn_in", "bits_in", "static", "ptr", "mask_in", "colsum_in", "dyn_out", "colsum_out", "bits_out", "current_out",
            "mask_out", "feature_out", "ratio_out", "nonbinary_out"]
# the fields a valid request of each form carries (the others stay null) ...
USED = {
    COPY: ["dyn_in", "static", "ptr", "mask_in", "colsum_in", "dyn_out", "colsum_out", "current_out", "mask_out", "feature_out", "ratio_out"],
    BITS: ["bits_in", "static", "ptr", "mask_in", "bits_out", "dyn_out", "current_out", "mask_out", "feature_out", "ratio_out"],
    FIRST: ["dyn_in", "static", "ptr", "mask_in", "bits_out", "dyn_out", "current_out", "mask_out", "feature_out", "ratio_out",
            "nonbinary_out"],
}
# ... and those it cannot do without (dyn_out is optional on the bit shadow: no fp32 expansion; mask_in: see the rows)
REQUIRED = {
    COPY: ["static", "ptr", "current_out", "mask_out", "dyn_in", "colsum_in", "dyn_out", "colsum_out"],
    BITS: ["static", "ptr", "current_out", "mask_out", "bits_in", "bits_out"],
    FIRST: ["static", "ptr", "current_out", "mask_out", "dyn_in", "bits_out"],
}
BAD = {COPY: "bad transition arguments", BITS: "bad transition_bits arguments", FIRST: "bad transition_first arguments"}
COMMON = "bad transition arguments"
# what tap_mask_step_bits / _first refuse as well, of the pointers above (ptr: update_rows = 3 needs it)
_MASK_STEP_NEEDS = {BITS: {"bits_in", "static", "ptr"}, FIRST: {"dyn_in", "bits_out", "static", "ptr"}}


@dataclass(frozen=True)
class Row:
    name: str
    form: int
    status: int
    message: str
    null: tuple = ()              # pointer fields (or "state") handed in as null
    ints: tuple = ()              # ((field, value), ...) over n, R, rows, update_rows, static_rows
    flags: int = 0
    alias: tuple = ()             # (a, b): field a is handed the buffer of field b
    from_stepper: bool = False    # the call comes from tap_stepper_step (host check only: the C ABI has no such entry)
    mask_step: bool = False       # tap_mask_step_bits / _first refuse these arguments too (TAP_E_INVALID)


def rows():
    out = []
    for form, fn in FORM_NAMES.items():
        own = lambda f: f in ("dyn_in", "colsum_in", "dyn_out", "colsum_out", "bits_in", "bits_out")
        for f in REQUIRED[form]:
            out.append(Row("%s-null-%s" % (fn, f), form, TAP_E_INVALID, BAD[form] if own(f) else COMMON, null=(f,),
                           mask_step=f in _MASK_STEP_NEEDS.get(form, ())))
        out.append(Row("%s-null-state" % fn, form, TAP_E_INVALID, COMMON, null=("state",)))
        for f in ("n", "R", "rows"):
            out.append(Row("%s-%s-0" % (fn, f), form, TAP_E_INVALID, COMMON, ints=((f, 0),), mask_step=form != COPY))
        out.append(Row("%s-static_rows-D" % fn, form, TAP_E_INVALID, COMMON, ints=(("static_rows", D),)))
        for v in (-1, 4):
            out.append(Row("%s-update_rows-%d" % (fn, v), form, TAP_E_INVALID, COMMON, ints=(("update_rows", v),), mask_step=form != COPY))
        out.append(Row("%s-ratio-without-ratio_out" % fn, form, TAP_E_INVALID, COMMON, null=("ratio_out",), flags=TAP_T_RATIO))
        # a public call needs mask_in; a stepper's first step may leave it null (= ones)
        out.append(Row("%s-public-null-mask_in" % fn, form, TAP_E_INVALID, COMMON, null=("mask_in",)))
        out.append(Row("%s-stepper-null-mask_in" % fn, form, TAP_OK, "", null=("mask_in",), from_stepper=True))
    out.append(Row("copy-dyn_in-is-dyn_out", COPY, TAP_E_INVALID, "transition is out of place (pack.py:370)", alias=("dyn_out", "dyn_in")))
    out.append(Row("first-dyn_in-is-dyn_out", FIRST, TAP_E_INVALID, BAD[FIRST], alias=("dyn_out", "dyn_in"), mask_step=True))
    out.append(Row("bits-bits_in-is-bits_out", BITS, TAP_E_INVALID, BAD[BITS], alias=("bits_out", "bits_in"), mask_step=True))
    return out


ROWS_TABLE = rows()


def ints_of(row):
    v = dict(n=N, R=R, rows=ROWS, update_rows=UPDATE_ROWS, static_rows=STATIC_ROWS)
    v.update(dict(row.ints))
    return v


def pointers_of(row, buffers):
    """{field: value} for the row: `buffers` maps every pointer field (and "state") to its valid value; unused and nulled
    fields come back as None, an aliased one as the other's value."""
    p = {f: (buffers[f] if f in USED[row.form] else None) for f in POINTERS}
    p["state"] = buffers["state"]
    for f in row.null:
        p[f] = None
    if row.alias:
        p[row.alias[0]] = p[row.alias[1]]
    return p
