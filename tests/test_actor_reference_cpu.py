"""The reference's own actor (model.DRL.forward, model.py:254-515; recorded by tests/golden/make_golden_actor.py) against the
package's modules, without a GPU: the whole state dict loads strictly into package modules, and the package's torch path
and its folds, teacher-forced on the recorded tour in float64, give the reference's logits, last_hh and tour_logp.

The bound is 1e-12 * max |want|: float64 arithmetic in another order (sums of at most 128 + 64 terms), not a measurement.
``Pointer.forward_step`` itself has no route without a device at Hd = 64 -- its torch path ends in the ``pointer_scores``
launch --, so the folds (``project_static``, ``fold_decoder(combine='cat')``, ``fold_episode``) are composed here through the
two launches' contracts in torch (decoder_step_model.step_torch, pointer_model.folded_torch); the GPU file runs
``forward_step``."""
import os

import numpy as np
import pytest
import torch

import actor_reference_cases as AC
import decoder_step_model as DM
import oracle_lib as O
import pointer_model as PM

BOUND = 1e-12


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _close(name, got, want):
    want = np.asarray(want, np.float64)
    err, top = float(np.abs(got.detach().numpy() - want).max()), float(np.abs(want).max())
    assert top > 0 and err <= BOUND * top, (name, err, top)
    return err / top


def _teacher_forced(D, ws, step):
    """the loop of model.py:342-515 on the recorded tour, float64: ``step(k, dyn (B, rows, nR), decoder_static,
    decoder_dynamic, last_hh or None)`` -> logits, last_hh (1, B, Hd); ``dynamic`` and both masks are rebuilt per step with
    the oracle and the decoder inputs are the fixture's.  Asserts logits, last_hh and tour_logp; -> worst err / max |want|"""
    z = AC.load(D, ws)
    st, dyn = AC.instances(D)
    tour = z["tour_idx"].astype(np.int64)
    B, n, R = AC.BATCH[D], AC.N, st.shape[2] // AC.N
    cur, mask = O.initial_mask(dyn, n), np.ones((B, st.shape[2]), np.float32)
    hh, worst = None, 0.0
    with torch.no_grad():
        for k in range(n):
            assert np.array_equal(cur, z["current_mask"][k].astype(np.float32)), k          # the mask this step's softmax saw
            logits, hh = step(k, _t(dyn), _t(z["decoder_static"][k]), _t(z["decoder_dynamic"][k]), hh)
            assert logits.dtype is torch.float64 and tuple(hh.shape) == (1, B, AC.HD)
            worst = max(worst, _close("logits %d" % k, logits, z["logits"][k]), _close("last_hh %d" % k, hh[0], z["last_hh"][k]))
            # model.py:359, 371-372: softmax(probs + current_mask.log()), the log of the value at the column
            logp = torch.log_softmax(logits + torch.log(_t(cur)), dim=1).gather(1, torch.from_numpy(tour[:, k:k + 1]))[:, 0]
            err = float((logp - _t(z["tour_logp"][:, k])).abs().max())
            assert err <= BOUND * max(1.0, float(np.abs(z["tour_logp"]).max())), (k, err)
            assert (cur[np.arange(B), tour[:, k]] == 1).all()
            dyn = O.update_dynamic(dyn, st, tour[:, k], n, 3)
            cur, mask = O.update_mask(mask, dyn, tour[:, k], n, R)
    assert not mask.any()
    return worst


@pytest.mark.parametrize("D,ws", AC.CASES)
def test_the_whole_state_dict_loads_strictly(D, ws):
    """nn.Conv1d (static_encoder.conv, static_decoder.conv, 2D dynamic_decoder.conv), DynamicBitsEncoder (dynamic_encoder),
    HeightmapEncoder (3D dynamic_decoder) and Pointer (pointer.*) take the reference's state dict between them: every load
    strict, no key left over, none taken twice, none invented"""
    z = AC.load(D, ws)
    sd = AC.state_dict(z)
    mods, taken = AC.build(z, D)
    assert taken == set(sd) and len(sd) == AC.N_KEYS[D]
    params = AC.named_parameters(mods)
    assert set(params) == set(sd)                                   # the reference's actor has no buffers
    for k, p in params.items():
        assert p.dtype is torch.float32 and torch.equal(p.detach(), sd[k]), k
        assert ("grad_" + k) in z and z["grad_" + k].shape == tuple(p.shape) and z["grad_" + k].dtype == np.float64
        assert np.abs(z["grad_" + k]).max() > 0 and z["e_ref_grad_" + k] >= 0, k


@pytest.mark.parametrize("D,ws", AC.CASES)
def test_torch_path_gives_the_references_numbers(D, ws):
    """static_encoder(static[:, 1:, :]), the decoder's two encoders concatenated, Pointer.forward on dynamic_encoder(dynamic),
    last_hh carried from step to step (None at step 0, as DRL.forward passes it on)"""
    mods, _ = AC.build(AC.load(D, ws), D)
    for m in mods.values():
        m.double()
    st, _ = AC.instances(D)
    static_hidden = mods["static_encoder.conv."](_t(st)[:, 1:, :])
    dec_s, dec_d, enc, pointer = mods["static_decoder.conv."], AC.dynamic_decoder(mods), mods["dynamic_encoder."], mods["pointer."]

    def step(k, dyn, ds, dd, hh):
        decoder_hidden = torch.cat((dec_s(ds), dec_d(dd)), 1)
        assert tuple(decoder_hidden.shape) == (AC.BATCH[D], AC.HD, 1)
        return pointer(static_hidden, enc(dyn), decoder_hidden, hh)
    print("torch path %dD %s: worst err / max |want| %.3g" % (D, ws, _teacher_forced(D, ws, step)))


@pytest.mark.parametrize("D,ws", AC.CASES)
def test_folds_give_the_references_numbers(D, ws):
    """project_static, fold_decoder(combine='cat') and fold_episode in float64, once per episode, then a step as the two
    launches' contracts state it: h', q from [decoder_static ; decoder_dynamic (2D) or the height-map encoder's output (3D,
    behind the fold's identity columns)] through P, c, w_hh, b_hh, Wq; the logits from proj, the 0/1 dynamic, M, k, q and
    the two v.  He != Hd, so a fold that sliced the two W by the wrong size fails here"""
    mods, _ = AC.build(AC.load(D, ws), D)
    for m in mods.values():
        m.double()
    st, _ = AC.instances(D)
    B, nR = st.shape[0], st.shape[2]
    dec_s, dec_d, enc, pointer = mods["static_decoder.conv."], AC.dynamic_decoder(mods), mods["dynamic_encoder."], mods["pointer."]
    with torch.no_grad():
        proj = pointer.project_static(mods["static_encoder.conv."](_t(st)[:, 1:, :]))
        P, c = pointer.fold_decoder(dec_s, dec_d, combine='cat')
        fold = pointer.fold_episode(enc, P, c)
    assert tuple(proj.shape) == (B, 3, nR, AC.HD) and tuple(fold.M.shape) == (3 * AC.HD, 3 * AC.N)
    assert tuple(fold.P.shape) == (3 * AC.HD, D + (4 if D == 2 else AC.HD // 2)) and (fold.heightmap is dec_d) == (D == 3)
    natural = proj.permute(0, 1, 3, 2).reshape(B, 3 * AC.HD, nR)              # pointer_model's (B, 3 Hd, nR)

    def step(k, dyn, ds, dd, hh):
        xd = dd[:, :, 0] if D == 2 else dec_d(dd)[:, :, 0]
        h_new, q, _ = DM.step_torch(ds[:, :, 0], xd, None if hh is None else hh[0], fold.P, fold.c, fold.w_hh, fold.b_hh, fold.Wq)
        return PM.folded_torch(natural, dyn, fold.M, fold.k, q, fold.va, fold.vp)[0], h_new.unsqueeze(0)
    print("folds %dD %s: worst err / max |want| %.3g" % (D, ws, _teacher_forced(D, ws, step)))


@pytest.mark.parametrize("D", [2, 3])
def test_the_fixtures_are_what_the_tests_need(D):
    """the batch crosses the decoder kernels' 16-env tile with a ragged second one; 'sharp' is 'init' times the stored
    factors and its logits lie in the range of the pretrained actor of that dimension (every step's max |logits| inside
    [0.5 x smallest, 2 x largest] of pretrained_logit_range), 'init' far below it; each file is smaller than the largest
    fixture committed before them"""
    init, sharp = AC.load(D, "init"), AC.load(D, "sharp")
    B = AC.BATCH[D]
    assert B > 16 and B % 16 != 0
    for z in (init, sharp):
        assert z["logits"].shape == (AC.N, B, AC.N * (2 if D == 2 else 6)) and z["last_hh"].shape == (AC.N, B, AC.HD)
        assert z["tour_idx"].shape == (B, AC.N) and z["tour_logp"].shape == (B, AC.N) and z["adv"].shape == (B,)
        assert z["e_ref_logits"].shape == (AC.N,) and z["e_ref_last_hh"].shape == (AC.N,) and z["e_ref_tour_logp"].shape == ()
        assert not z["decoder_static"][0].any() and not z["decoder_dynamic"][0].any()       # step 0 sees zeros
        assert z["decoder_static"][1:].any() and z["decoder_dynamic"][1:].any()
    for ws in ("init", "sharp"):
        assert os.path.getsize(AC.path(D, ws)) < AC.SIZE_LIMIT
    lo, hi = sharp["pretrained_logit_range"]
    assert np.array_equal(init["pretrained_logit_range"], sharp["pretrained_logit_range"]) and 0 < lo <= hi
    peaks = np.abs(sharp["logits"]).max(axis=(1, 2))
    assert (peaks >= 0.5 * lo).all() and (peaks <= 2.0 * hi).all(), (peaks, lo, hi)
    assert np.abs(init["logits"]).max() < 1.0                       # the linear part of tanh, a flat softmax
    fv, fw = (np.float32(v) for v in sharp["sharp_factors"])
    for k in (k for k in init if k.startswith("sd_")):
        name = k[len("sd_"):]
        f = fv if name in ("pointer.v", "pointer.encoder_attn.v") else fw if name.startswith("pointer.") and init[k].ndim > 1 \
            else np.float32(1)
        assert np.array_equal(sharp[k], init[k] * f), k
    assert np.array_equal(init["adv"], sharp["adv"])
    print("%dD: pretrained per-step max |logits| %.4g .. %.4g, sharp %.4g .. %.4g (factors %g, %g), init %.3g" % (
        D, lo, hi, peaks.min(), peaks.max(), fv, fw, np.abs(init["logits"]).max()))
