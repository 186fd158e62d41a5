"""The fused pointer launch on the MI355X (pointer.hip: k_pointer_scores<HPL, SS, PtrArgsPick, FORM>; tapenv.h:
tap_pointer_pick_static) against the composition it replaces: ``pointer_scores_static`` followed by the head.  BYTES: ``ptr``
equal, ``logp`` bit-equal with NaN rows matching as NaN, and ``logits_out``, when asked for, the static-rows launch's logits.
Both forms (greedy, DRAW -- through a record and through a StepDropout at two steps), ``xs`` contiguous and as the
``[:, 1:, :]`` view of a (B, S + 1, nR) tensor, random shadows and masks with a few rows forced empty, at
rolling_actor_model.SHAPES: every instantiation family (HPL 1 / 2, S in registers and in the LDS, one and two shadow planes), the
head's second chunk, and the two geometries with more than one env per workgroup."""
import numpy as np
import pytest
import torch

import actor_reference_cases as AC
import rolling_actor_model as RM
import tap_net_amd as T
from tap_net_amd import _lib, pack, rollout, tools

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, EPISODE, STEP, OFFSET = (0x5EED << 32) | 77, 3, 4, 9
GREEDY, DRAW = 1, 2                                             # the launch record's FORM field


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits32(t):
    return t.view(torch.int32) if t.dtype is torch.float32 else t


def _bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits32(a), _bits32(b))


_CASES = {}


def _case(shape):
    """the case's device tensors and the composition's logits, made once and left unchanged"""
    if shape not in _CASES:
        B, nR, rows, Hd, S = shape
        X = RM.make_case(B, nR, rows, Hd, S, seed=RM.SHAPES.index(shape))
        d = {k: _dev(X[k]) for k in ("xs", "bits", "G", "g", "M", "k", "q", "va", "vp", "mask")}
        wide = torch.full((B, S + 1, nR), float('nan'), device=DEV)          # row 0 is never read
        wide[:, 1:, :] = d["xs"]
        d["view"] = wide[:, 1:, :]
        d["logits"] = T.pointer_scores_static(d["xs"], d["bits"], d["G"], d["g"], d["M"], d["k"], d["q"], d["va"], d["vp"], rows=rows)
        d["empty"] = [b for b in RM.EMPTY_ROWS if b < B]
        assert not d["view"].is_contiguous() and int((d["mask"].sum(1) == 0).sum()) == len(d["empty"])
        _CASES[shape] = d
    return _CASES[shape]


def _fused(d, rows, xs, source=None, want_logits=False):
    return T.pointer_pick_static(xs, d["bits"], d["G"], d["g"], d["M"], d["k"], d["q"], d["va"], d["vp"], d["mask"], source,
                                 rows=rows, want_logits=want_logits)


def _state():
    return torch.tensor([SEED, EPISODE], dtype=torch.int64, device=DEV)


def _same(got, want, d):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert _bytes(a, b)
    assert bool(torch.isnan(got[1][d["empty"]]).all()) and not bool(got[0][d["empty"]].any())
    live = torch.ones_like(got[1], dtype=torch.bool)
    live[d["empty"]] = False
    assert bool(torch.isfinite(got[1][live]).all())
    assert bool((d["mask"].gather(1, got[0].unsqueeze(1))[:, 0][live] != 0).all())          # every pick is selectable


@pytest.mark.parametrize("shape", RM.SHAPES, ids=["-".join(str(v) for v in s) for s in RM.SHAPES])
def test_fused_launch_writes_the_compositions_bytes(shape):
    B, nR, rows, Hd, S = shape
    d = _case(shape)
    geo = _lib.pointer_scores_geometry(B, nR, rows, Hd, S)
    assert geo[0] == max(1, B // 1024) and geo[2] <= 60 * 1024, geo
    for name in ("xs", "view"):
        xs = d[name]
        _lib.variant_hits_reset(DEV)
        # greedy
        want = T.pointer_pick(d["logits"], d["mask"])
        got = _fused(d, rows, xs)
        _same(got, want, d)
        full = _fused(d, rows, xs, want_logits=True)
        _same(full[:2], want, d)
        assert _bytes(full[2], d["logits"])
        _same(_fused(d, rows, xs), got, d)                                               # two calls, the same bytes
        # DRAW at a record
        rec = rollout.PickRecord(_state(), STEP, OFFSET)
        want = T.pointer_pick_draw(d["logits"], d["mask"], rec)
        got = _fused(d, rows, xs, rec)
        _same(got, want, d)
        full = _fused(d, rows, xs, (rec.state, STEP, OFFSET), want_logits=True)
        _same(full[:2], want, d)
        assert _bytes(full[2], d["logits"])
        _same(_fused(d, rows, xs, rec), got, d)
        # DRAW through a StepDropout at two steps: the fused launch takes the pick records the head would take
        a, b = tools.StepDropout(SEED & 0xFFFF, DEV, OFFSET), tools.StepDropout(SEED & 0xFFFF, DEV, OFFSET)
        a.next_episode(), b.next_episode()
        for _ in range(2):
            want = T.pointer_pick_draw(d["logits"], d["mask"], a)
            got = _fused(d, rows, xs, b)
            _same(got, want, d)
        assert a.pick == b.pick == 2
        torch.cuda.synchronize()
        planes, hpl = (2, 1) if rows > 64 else (1, 2 if Hd > 64 else 1)
        keys = {k for k in _lib.variant_keys(DEV) if k[0] == _lib.TAP_HIT_POINTER and k[1] != 0}
        assert keys == {(_lib.TAP_HIT_POINTER, f, hpl, planes, Hd // (64 * hpl), 0, S) for f in (GREEDY, DRAW)}, keys


def test_model_agrees_on_the_small_shape():
    """the numpy model of the fused launch (fp32 scores, fp64 head) on c5's window: the picks agree wherever the model's pick is
    not a near-tie of the fp32 logits, and logp is within the fp32 scores' error"""
    shape = RM.SHAPES[0]
    B, nR, rows, Hd, S = shape
    X = RM.make_case(B, nR, rows, Hd, S, seed=0)
    d = _case(shape)
    ptr, logp, logits = RM.fused(X["xs"], X["G"], X["g"], X["dyn"], X["M"], X["k"], X["q"], X["va"], X["vp"], X["mask"])
    got = _fused(d, rows, d["xs"], want_logits=True)
    gl = got[2].cpu().numpy().astype(np.float64)
    err = float(np.abs(gl - logits).max())
    print("fused logits against the float64 model: err %.3g" % err)
    assert err <= 1e-4
    live = [b for b in range(B) if b not in d["empty"]]
    sel = np.where(X["mask"] != 0, logits, -np.inf)
    top2 = np.sort(sel, 1)[:, -2:]
    clear = [b for b in live if X["mask"][b].sum() == 1 or top2[b, 1] - top2[b, 0] > 4 * err]
    assert len(clear) >= len(live) // 2
    assert np.array_equal(got[0].cpu().numpy()[clear], ptr[clear])
    assert float(np.abs(got[1].cpu().numpy()[clear].astype(np.float64) - logp[clear]).max()) <= 4 * err + 1e-6


def test_wrapper_refusals():
    shape = RM.SHAPES[0]
    B, nR, rows, Hd, S = shape
    d = _case(shape)
    with pytest.raises(ValueError):                                  # no backward
        g = d["G"].clone().requires_grad_(True)
        T.pointer_pick_static(d["xs"], d["bits"], g, d["g"], d["M"], d["k"], d["q"], d["va"], d["vp"], d["mask"], rows=rows)
    with torch.no_grad():                                            # ... but fine where nothing records
        g = d["G"].clone().requires_grad_(True)
        out = T.pointer_pick_static(d["xs"], d["bits"], g, d["g"], d["M"], d["k"], d["q"], d["va"], d["vp"], d["mask"], rows=rows)
        assert _bytes(out[0], T.pointer_pick(d["logits"], d["mask"])[0])
    with pytest.raises(ValueError):
        T.pointer_pick_static(d["xs"], d["bits"], d["G"], d["g"], d["M"], d["k"], d["q"], d["va"], d["vp"], d["mask"][:, :-1], rows=rows)
    with pytest.raises(TypeError):
        T.pointer_pick_static(d["xs"], d["bits"].float(), d["G"], d["g"], d["M"], d["k"], d["q"], d["va"], d["vp"], d["mask"], rows=rows)
    # a view the launch cannot read in place is copied, not refused: the transposed rows
    odd = d["xs"].transpose(1, 2).contiguous().transpose(1, 2)
    assert rollout._rows_view_stride(odd) is None
    _same(_fused(d, rows, odd), T.pointer_pick(d["logits"], d["mask"]), d)
    assert T.pointer_pick_static_supported(rows, nR, Hd, S) and not T.pointer_pick_static_supported(rows, nR, 96, S)
    assert not T.pointer_pick_static_supported(rows, nR, Hd, 9) and not T.pointer_pick_static_supported(rows, 6, Hd, S)


@pytest.mark.parametrize("D", [2, 3])
def test_forward_step_pick_is_forward_step_and_the_head(D):
    """Pointer.forward_step_pick on the reference's actor (2D: the plain decoder step; 3D: the height-map one) at two steps of an
    episode, greedy and DRAW, with the window's static rows passed as a view: the bytes of forward_step + pointer_pick[_draw],
    in two launches of which none is the head's; a proj tensor and grad mode take today's launches"""
    z = AC.load(D, "sharp")
    actor = T.DRL(D, 3 * AC.N, AC.HE, AC.HD, True, 'bot', True, 5, 50, D, "C+P+S-lb-soft", 'shape_heightmap', "diff", "LB_GREEDY",
                  pack.update_dynamic, pack.update_mask, 1, 0.)
    actor.load_state_dict(AC.state_dict(z), strict=True)
    actor = actor.to(DEV).eval()
    st, dy = AC.instances(D)
    static, dynamic = _dev(st), _dev(dy)
    B = int(static.shape[0])
    pointer = actor.pointer
    with torch.no_grad():
        sp = actor._own_stepper(static, dynamic, AC.N)
        sp.begin(static, dynamic)
        base = pointer.fold_static(actor.static_encoder, static[:, 1:, :])
        P, c = pointer.fold_decoder(actor.static_decoder, actor.dynamic_decoder, combine='cat')
        fold = pointer.fold_episode(actor.dynamic_encoder, P, c)
        ds = torch.zeros(B, D, 1, device=DEV)
        dd = torch.zeros((B, 4, 1) if D == 2 else (B, 2, 5, 5), device=DEV)
        hh = None
        for step in range(2):
            sf = base.with_rows(static[:, 1:, :])
            assert sf.xs.data_ptr() == static[:, 1:, :].data_ptr() and sf.G is base.G
            bits, cur = sp.dynamic_bits, sp.current_mask
            logits, hh_want = pointer.forward_step(base, bits, fold, ds, dd, hh)
            want = T.pointer_pick(logits, cur)
            rec = rollout.PickRecord(_state(), step, OFFSET)
            want_draw = T.pointer_pick_draw(logits, cur, rec)
            _lib.variant_hits_reset(DEV)
            ptr, logp, hh_got = pointer.forward_step_pick(sf, bits, fold, ds, dd, hh, cur)
            torch.cuda.synchronize()
            hits = _lib.variant_hits(DEV)
            assert sum(v for k, v in hits.items() if k[0] == _lib.TAP_HIT_POLICY_PICK) == 0
            assert sum(v for k, v in hits.items() if k[0] == _lib.TAP_HIT_POINTER) == 1
            assert sum(v for k, v in hits.items() if k[0] == (_lib.TAP_HIT_DECODER if D == 2 else _lib.TAP_HIT_HEIGHTMAP)) == 1
            assert _bytes(ptr, want[0]) and _bytes(logp, want[1]) and _bytes(hh_got, hh_want)
            out = pointer.forward_step_pick(sf, bits, fold, ds, dd, hh, cur, rec, want_logits=True)
            assert _bytes(out[0], want_draw[0]) and _bytes(out[1], want_draw[1]) and _bytes(out[2], logits) and _bytes(out[3], hh_want)
            # a proj tensor: today's two launches and the head's
            proj = pointer.project_static(actor.static_encoder(static[:, 1:, :]))
            _lib.variant_hits_reset(DEV)
            p2 = pointer.forward_step_pick(proj, bits, fold, ds, dd, hh, cur)
            torch.cuda.synchronize()
            assert sum(v for k, v in _lib.variant_hits(DEV).items() if k[0] == _lib.TAP_HIT_POLICY_PICK) == 1
            assert bool(torch.isfinite(p2[1]).all())
            hh = hh_want
            sp.step(ptr)
            ds, dd = sp.decoder_static, sp.decoder_dynamic
    # grad enabled and parameters that require it: forward_step and the head, differentiable
    with torch.enable_grad():
        sp.begin(static, dynamic)
        base = pointer.fold_static(actor.static_encoder, static[:, 1:, :])
        P, c = pointer.fold_decoder(actor.static_decoder, actor.dynamic_decoder, combine='cat')
        fold = pointer.fold_episode(actor.dynamic_encoder, P, c)
        ptr, logp, _ = pointer.forward_step_pick(base.with_rows(static[:, 1:, :]), sp.dynamic_bits, fold,
                                                 torch.zeros(B, D, 1, device=DEV),
                                                 torch.zeros((B, 4, 1) if D == 2 else (B, 2, 5, 5), device=DEV), None, sp.current_mask)
        assert logp.requires_grad
