"""Dropout inside the decoder step without a GPU: the generator's known answers, the torch form of the masks
(rollout.dropout_keep_words) against the numpy model (tests/step_dropout_model.py) bit for bit, the masks' statistics,
``tools.StepDropout``, ``Pointer.forward_step_dropout``'s torch path in float64 against a hand-written step, and the
exports."""
import copy
import inspect
import re

import numpy as np
import pytest
import torch
from torch import nn

import step_dropout_model as SD
import tap_net_amd as T
from tap_net_amd import _lib, rollout, tools

# counter, key -> output (Random123's known answers for philox4x32-10, recomputed with the numpy model)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _state(seed, episode):
    return torch.tensor([seed, episode], dtype=torch.int64)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answers(counter, key, want):
    assert tuple(int(w) for w in SD.philox4x32_10(counter, key)) == want
    got = rollout.philox4x32_10([torch.tensor([v], dtype=torch.int64) for v in counter], [torch.tensor([v], dtype=torch.int64) for v in key])
    assert tuple(int(w) for w in got) == want


def test_known_answers_through_the_keep_words():
    """env 0, row 0, step 0, episode 0, seed 0 is the all-zero counter and key: word 0 = 6627e8d5 decides drop_rnn and word
    1 = e169c58d drop_hh, and keep iff word >= thr.  p = w / 2^32 is exact in a double, so thr = w"""
    for plane, word in ((0, 0x6627e8d5), (1, 0xe169c58d)):
        for thr, kept in ((word, 1), (word + 1, 0)):
            p = [0.0, 0.0]
            p[plane] = thr / 2.0 ** 32
            assert rollout.dropout_threshold(p[plane]) == thr
            w = rollout.dropout_keep_words(_state(0, 0), 0, 1, 64, p[0], p[1])
            assert int(w[0, plane, 0]) & 1 == kept and int(w[0, 1 - plane, 0]) == -1
    # where the counter's and the key's words come from: env_offset + b, the row, the step, the episode; the seed's halves
    # (a row index is below Hd, so the other two known answers cannot be reached through the masks)
    c, k = (7, 5, 3, 9), (0x89ABCDEF, 0x01234567)
    word = SD.philox4x32_10(c, k)
    for plane in (0, 1):
        for thr, kept in ((int(word[plane]), 1), (int(word[plane]) + 1, 0)):
            p = [0.0, 0.0]
            p[plane] = thr / 2.0 ** 32
            w = rollout.dropout_keep_words(_state(k[0] | (k[1] << 32), c[3]), c[2], 3, 64, p[0], p[1], env_offset=c[0] - 2)
            assert (int(w[2, plane, 0]) >> c[1]) & 1 == kept


@pytest.mark.parametrize("B,Hd", [(1, 64), (67, 128), (5, 256)])
def test_keep_words_equal_the_numpy_model(B, Hd):
    seed = 0x1234567855AA33CC
    for env_offset in (0, 1000):
        for step in (0, 3):
            for episode in (0, 2 ** 32 + 1):                       # the counter takes the episode mod 2^32
                got = rollout.dropout_keep_words(_state(seed, episode), step, B, Hd, 0.1, 0.3, env_offset)
                want = SD.keep_words(seed, episode, step, B, Hd, 0.1, 0.3, env_offset)
                assert got.dtype is torch.int64 and tuple(got.shape) == (B, 2, Hd // 64)
                assert np.array_equal(got.numpy(), want), (env_offset, step, episode)
                assert np.array_equal(rollout.dropout_keep_mask(got).numpy(), SD.keep_bool(seed, episode, step, B, Hd, 0.1, 0.3, env_offset))
    assert np.array_equal(SD.keep_words(seed, 2 ** 32 + 1, 0, B, Hd, 0.1, 0.3), SD.keep_words(seed, 1, 0, B, Hd, 0.1, 0.3))
    assert not np.array_equal(SD.keep_words(seed, 0, 0, B, Hd, 0.1, 0.3), SD.keep_words(seed, 1, 0, B, Hd, 0.1, 0.3))
    # an env's masks do not depend on the batch: rows 1000 .. of a larger call
    big = rollout.dropout_keep_words(_state(seed, 0), 3, 1000 + B, Hd, 0.1, 0.3)
    assert torch.equal(big[1000:], rollout.dropout_keep_words(_state(seed, 0), 3, B, Hd, 0.1, 0.3, 1000))


def test_p_zero_keeps_everything_and_the_thresholds():
    w = rollout.dropout_keep_words(_state(7, 3), 2, 5, 128, 0.0, 0.0)
    assert bool((w == -1).all())
    assert [rollout.dropout_threshold(p) for p in (0.1, 0.3, 0.5)] == [429496730, 1288490189, 2147483648]
    assert [SD.threshold(p) for p in (0.1, 0.3, 0.5)] == [429496730, 1288490189, 2147483648]
    assert rollout.dropout_threshold(0.0) == 0 and rollout.dropout_threshold(1.0) == 2 ** 32 - 1
    assert rollout.dropout_scale(0.0) == 1.0 and rollout.dropout_scale(0.1) == float(np.float32(1 / 0.9)) == SD.scale(0.1)
    with pytest.raises(ValueError):
        rollout.dropout_threshold(1.5)
    with pytest.raises(ValueError):
        rollout.dropout_keep_words(_state(0, 0), 0, 2, 96, 0.1, 0.1)
    with pytest.raises(ValueError):
        rollout.dropout_keep_words(torch.zeros(2), 0, 2, 64, 0.1, 0.1)


def test_keep_fractions():
    """seed 12345, B = 2051, Hd = 256, steps 0 .. 3 of episode 0: N = 2 100 224 draws per mask.  The keep fraction of a fair
    generator lies within 4 sigma = 4 sqrt(p (1 - p) / N) of 1 - p but for 6e-5 of the time; two independent masks at p = 0.5
    agree on half of the elements, 0.50 +- 0.01 being 29 sigma wide"""
    B, Hd, steps = 2051, 256, 4
    N = B * Hd * steps
    state = _state(12345, 0)
    halves = None
    for p in (0.1, 0.3, 0.5):
        masks = torch.stack([rollout.dropout_keep_mask(rollout.dropout_keep_words(state, t, B, Hd, p, p)) for t in range(steps)])
        assert masks.shape == (steps, B, 2, Hd)
        for plane in (0, 1):
            frac = float(masks[:, :, plane].double().mean())
            sigma = np.sqrt(p * (1 - p) / N)
            print("keep fraction p %.1f plane %d: %.6f, %.2f sigma from %.1f" % (p, plane, frac, (frac - (1 - p)) / sigma, 1 - p))
            assert abs(frac - (1 - p)) <= 4 * sigma, (p, plane, frac)
        halves = masks
    rnn_hh = float((halves[:, :, 0] == halves[:, :, 1]).double().mean())
    steps01 = float((halves[0] == halves[1]).double().mean())
    print("agreement at p 0.5: rnn / hh %.4f, step 0 / step 1 %.4f" % (rnn_hh, steps01))
    assert abs(rnn_hh - 0.5) <= 0.01 and abs(steps01 - 0.5) <= 0.01


def test_step_dropout_object():
    a, b = T.StepDropout(99, "cpu"), T.StepDropout(99, "cpu")
    assert a.state.dtype is torch.int64 and a.state.tolist() == [99, 0] and a.step == 0 and a.env_offset == 0
    r0, r1 = a.take_step(0.1, 0.3), a.take_step(0.1, 0.3)
    assert (r0.step, r1.step, a.step) == (0, 1, 2) and r0.state is a.state and (r0.p_rnn, r0.p_hh, r0.env_offset) == (0.1, 0.3, 0)
    words = lambda r, B=6: rollout.dropout_keep_words(r.state, r.step, B, 64, r.p_rnn, r.p_hh, r.env_offset)
    first = words(r0)
    assert torch.equal(first, words(b.take_step(0.1, 0.3))) and not torch.equal(first, words(r1))     # one seed: one stream
    a.next_episode()
    assert a.state.tolist() == [99, 1] and a.step == 0
    again = a.take_step(0.1, 0.3)
    assert again.step == 0 and not torch.equal(words(again), first)                                    # a new episode: new masks
    assert np.array_equal(words(again).numpy(), SD.keep_words(99, 1, 0, 6, 64, 0.1, 0.3))
    shard = T.StepDropout(99, "cpu", env_offset=4)
    assert torch.equal(words(shard.take_step(0.1, 0.3), 2), first[4:])                                 # rows 4 .. of the larger batch
    with pytest.raises(ValueError):
        T.StepDropout(-1, "cpu")
    with pytest.raises(ValueError):
        T.StepDropout(1, "cpu", env_offset=-1)


# ---- Pointer.forward_step_dropout on the CPU ------------------------------------------------------------------------
HD, B_, NR, ROWS = 64, 5, 10, 10            # rows 10 x nR 10 has no bit shadow: forward_bits is ``forward`` on the float dynamic
P_RNN, P_HH = 0.1, 0.3                      # unequal: swapped masks would show


def _net(seed=5):
    torch.manual_seed(seed)
    net = tools.Pointer(HD, HD, 'shape_heightmap', 'bot').double()
    for p in net.parameters():
        nn.init.xavier_uniform_(p) if p.dim() > 1 else nn.init.normal_(p, std=0.1)
    net.drop_rnn.p, net.drop_hh.p = P_RNN, P_HH
    enc = T.DynamicBitsEncoder(ROWS, HD).double()
    dec_s, dec_d = nn.Conv1d(2, HD // 2, 1).double(), nn.Conv1d(4, HD // 2, 1).double()
    return net, enc, dec_s, dec_d


def _inputs(seed=6):
    g = torch.Generator().manual_seed(seed)
    sh = torch.randn(B_, HD, NR, generator=g).double()
    dyn = (torch.rand(B_, ROWS, NR, generator=g) < 0.3).double()
    ds = torch.randint(0, 6, (B_, 2, 1), generator=g).double()
    dd = torch.randint(0, 51, (B_, 4, 1), generator=g).double()
    hh = torch.tanh(torch.randn(1, B_, HD, generator=g)).double()
    return sh, dyn, ds, dd, hh


def _by_hand(net, enc, dec_s, dec_d, sh, dyn, ds, dd, hh, keep):
    """one decoding step written out: the folded GRU step of decoder_step_model with the masks, then the attention and the
    pointer as model.py:55-74 and 117-138 have them -> logits (B, nR), last_hh (1, B, Hd)"""
    P, c = net.fold_decoder(dec_s, dec_d)
    _, _, Wq = net.folded_weights()
    h_out, _, _, rnn = SD.step_torch(ds[:, :, 0], dd[:, :, 0], None if hh is None else hh[0], P, c, net.gru.weight_hh_l0,
                                     net.gru.bias_hh_l0, Wq, keep, P_RNN, P_HH)
    enc_h = torch.cat((sh, enc(dyn)), 1)                                                       # (B, 2 He, nR)
    hidden = torch.cat((enc_h, rnn.unsqueeze(2).expand(-1, -1, NR)), 1)
    at = net.encoder_attn
    attn = torch.softmax(torch.einsum('h,bhn->bn', at.v[0, 0], torch.tanh(torch.einsum('hk,bkn->bhn', at.W[0], hidden))), dim=1)
    context = torch.einsum('bn,bkn->bk', attn, enc_h).unsqueeze(2).expand_as(enc_h)
    energy = torch.cat((enc_h, context), 1)
    logits = torch.einsum('h,bhn->bn', net.v[0, 0], torch.tanh(torch.einsum('hk,bkn->bhn', net.W[0], energy)))
    return logits, h_out.unsqueeze(0)


def test_forward_step_dropout_on_the_cpu_equals_the_hand_written_step():
    net, enc, dec_s, dec_d = _net()
    net.train()
    sh, dyn, ds, dd, hh = _inputs()
    sd = T.StepDropout(31, "cpu", env_offset=2)
    sd.next_episode()
    with torch.no_grad():
        proj = net.project_static(sh)
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
        for t, last in enumerate((hh, None)):
            keep = SD.keep_bool(31, 1, t, B_, HD, P_RNN, P_HH, 2)
            assert keep[:, 0].sum() > keep[:, 1].sum() > 0 and not keep[:, 1].all()
            got = net.forward_step_dropout(proj, dyn, fold, ds, dd, last, sd)
            want = _by_hand(net, enc, dec_s, dec_d, sh, dyn, ds, dd, last, torch.from_numpy(keep))
            assert sd.step == t + 1 and tuple(got[1].shape) == (1, B_, HD)
            for g, w in zip(got, want):
                assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max())
            dropped = ~torch.from_numpy(keep[:, 1])
            assert bool((got[1][0][dropped] == 0).all()) and bool((got[1][0][~dropped] != 0).all())
            # forward_bits_dropout on the unfolded decoder_hidden is the same function of the same masks
            sd.step = t
            hidden = torch.cat((dec_s(ds), dec_d(dd)), 1)
            bits = net.forward_bits_dropout(proj, dyn, enc, hidden, last, sd)
            assert torch.equal(bits[0], got[0]) and torch.equal(bits[1], got[1])
        # torch's generator was never touched
        s0 = torch.random.get_rng_state()
        net.forward_step_dropout(proj, dyn, fold, ds, dd, hh, sd)
        assert torch.equal(s0, torch.random.get_rng_state())


def test_eval_ignores_the_dropout_source():
    net, enc, dec_s, dec_d = _net()
    net.eval()
    sh, dyn, ds, dd, hh = _inputs()
    sd = T.StepDropout(31, "cpu")
    with torch.no_grad():
        proj = net.project_static(sh)
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
        want = net.forward_step(proj, dyn, fold, ds, dd, hh)
        got = net.forward_step_dropout(proj, dyn, fold, ds, dd, hh, sd)
        bits = net.forward_bits_dropout(proj, dyn, enc, torch.cat((dec_s(ds), dec_d(dd)), 1), hh, sd)
    assert sd.step == 0
    for g in (got, bits):
        assert torch.equal(g[0], want[0]) and torch.equal(g[1], want[1])


def test_p_one_drops_everything_on_the_torch_path():
    net, enc, dec_s, dec_d = _net()
    net.train()
    net.drop_hh.p = 1.0
    sh, dyn, ds, dd, hh = _inputs()
    with torch.no_grad():
        proj = net.project_static(sh)
        fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
        logits, last = net.forward_step_dropout(proj, dyn, fold, ds, dd, hh, T.StepDropout(1, "cpu"))
    assert not bool(last.any()) and bool(torch.isfinite(logits).all())


def test_gradients_through_three_steps():
    """every parameter's gradient through a 3-step loop of forward_step_dropout against autograd through the hand-written
    form: float64, 1e-10 of the largest wanted value (three steps of sums of a few hundred terms of O(1))"""
    mods = _net()
    for m in mods:
        m.train()
    sh, dyn, ds, dd, hh = _inputs()
    g = torch.Generator().manual_seed(9)
    gl, gh = torch.randn(3, B_, NR, generator=g).double(), torch.randn(1, B_, HD, generator=g).double()

    def loss(stepper):
        last, total = hh, 0
        for t in range(3):
            logits, last = stepper(t, last)
            total = total + (logits * gl[t]).sum()
        return total + (last * gh).sum()

    def grads(ms):
        return {"%d.%s" % (i, n): p.grad.clone() for i, m in enumerate(ms) for n, p in m.named_parameters()}
    mine = copy.deepcopy(mods)
    sd = T.StepDropout(77, "cpu")
    net, enc, dec_s, dec_d = mine
    proj = net.project_static(sh)
    fold = net.fold_episode(enc, *net.fold_decoder(dec_s, dec_d))
    loss(lambda t, last: net.forward_step_dropout(proj, dyn, fold, ds + t, dd - t, last, sd)).backward()
    hand = copy.deepcopy(mods)
    loss(lambda t, last: _by_hand(*hand, sh, dyn, ds + t, dd - t, last,
                                  torch.from_numpy(SD.keep_bool(77, 0, t, B_, HD, P_RNN, P_HH)))).backward()
    got, want = grads(mine), grads(hand)
    assert sorted(got) == sorted(want) and len(got) == 8 + 2 + 2 + 2
    for name in sorted(want):
        assert float(want[name].abs().max()) > 0, name
        assert float((got[name] - want[name]).abs().max()) <= 1e-10 * float(want[name].abs().max()), name


def test_training_loop_model_equals_the_pointer_with_keep_words():
    """step_dropout_model.train_step's mask modules and Pointer._gru_step(keep=) are two writings of one function"""
    net, _, _, _ = _net()
    net.train()
    g = torch.Generator().manual_seed(3)
    hidden, hh = torch.randn(B_, HD, 1, generator=g).double(), torch.randn(1, B_, HD, generator=g).double()
    keep = SD.keep_bool(5, 0, 2, B_, HD, P_RNN, P_HH)
    other = copy.deepcopy(net)
    other.drop_rnn, other.drop_hh = SD.MaskDrop(P_RNN), SD.MaskDrop(P_HH)
    other.drop_rnn.kept, other.drop_hh.kept = torch.from_numpy(keep[:, 0]), torch.from_numpy(keep[:, 1])
    with torch.no_grad():
        a = net._gru_step(hidden, hh, torch.from_numpy(SD.pack(keep)))
        b = other._gru_step(hidden, hh)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- the exports ----------------------------------------------------------------------------------------------------
NEW = ("tap_decoder_step_dropout", "tap_decoder_step_hm_dropout", "tap_decoder_step_dropout_backward")


def test_exports_and_signatures():
    L = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(tap_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(L, name)
    assert declared == set(_lib.EXPORTS) and L.tap_abi_version() == 1
    assert [len(_lib._PROTOS[n][1]) for n in NEW] == [26, 36, 14]
    for name in ("decoder_step_dropout", "decoder_step_heightmap_dropout", "dropout_keep_words", "StepDropout"):
        assert name in T.__all__ and getattr(T, name) is not None
    assert list(inspect.signature(T.decoder_step_dropout).parameters) == ["xs", "xd", "h", "P", "c", "w_hh", "b_hh", "wq", "dropout"]
    assert list(inspect.signature(T.decoder_step_heightmap_dropout).parameters) == [
        "xs", "hm", "h", "encoder", "P", "c", "w_hh", "b_hh", "wq", "dropout"]
    assert list(inspect.signature(T.Pointer.forward_step_dropout).parameters) == [
        "self", "proj", "bits", "fold", "decoder_static", "decoder_dynamic", "last_hh", "dropout"]
    assert list(inspect.signature(rollout.dropout_keep_words).parameters) == ["state", "step", "B", "Hd", "p_rnn", "p_hh", "env_offset"]


def test_host_side_checks_need_no_device():
    """the new entries' argument checks in the existing entries' order, with a null context and host addresses that are
    never dereferenced: a null state or keep buffer is TAP_E_INVALID, and both are 8-byte aligned"""
    L = _lib.lib()
    inv, ok, uns = _lib.TAP_E_INVALID, _lib.TAP_OK, _lib.TAP_E_UNSUPPORTED
    buf = np.zeros(64, np.float64)
    p = _lib._vp(buf.ctypes.data)
    off4 = _lib._vp(buf.ctypes.data + 4)
    B, Hd = 2, 64

    def fwd(B, Ks, Kd, Hd, ins, state, outs):
        return L.tap_decoder_step_dropout(None, ins[0], Ks, ins[1], Kd, ins[2], B, Hd, *ins[3:8], state, 0, 0, 0, 0, 1.0, 1.0, *outs, None)
    ins, outs = [p] * 8, [p] * 5                                     # outs: h_out, q_out, gates_out, rnn_out, keep_out
    assert fwd(-1, 2, 4, Hd, ins, p, outs) == inv and fwd(B, 2, 4, 0, ins, p, outs) == inv
    assert fwd(0, 2, 4, Hd, [None] * 8, None, [None] * 5) == ok
    assert fwd(B, 2, 4, Hd, ins, None, outs) == inv and fwd(B, 2, 4, 96, ins, None, outs) == inv     # null comes before the shape
    assert fwd(B, 2, 4, Hd, ins, p, outs[:4] + [None]) == inv
    assert fwd(B, 2, 4, 96, ins, p, outs) == uns
    assert fwd(B, 2, 4, Hd, ins, off4, outs) == inv and fwd(B, 2, 4, Hd, ins, p, outs[:4] + [off4]) == inv
    assert fwd(B, 2, 4, Hd, ins, p, [p, p, p, _lib._vp(buf.ctypes.data + 2), p]) == inv                 # rnn_out: 4-byte

    def hm(B, Hd, m, state, keep):
        return L.tap_decoder_step_hm_dropout(None, p, 3, p, 2, 5, 5, p, B, Hd, m, *([p] * 11), state, 0, 0, 0, 0, 1.0, 1.0, p, p, p, p, p,
                                             keep, None)
    assert hm(-1, Hd, 32, p, p) == inv and hm(0, Hd, 32, None, None) == ok
    assert hm(B, Hd, 32, None, p) == inv and hm(B, Hd, 32, p, None) == inv and hm(B, Hd, 48, p, p) == uns
    assert hm(B, Hd, 32, off4, p) == inv and hm(B, Hd, 32, p, off4) == inv

    def bwd(B, Hd, bufs, keep):
        return L.tap_decoder_step_dropout_backward(None, B, Hd, *bufs[:4], keep, 1.0, 1.0, *bufs[4:], None)
    seven = [p] * 7                                                 # gates, h, g_h, g_r | dgi, dghn, carry
    assert bwd(-1, Hd, seven, p) == inv and bwd(B, 0, seven, p) == inv and bwd(0, Hd, [None] * 7, None) == ok
    for hole in range(7):
        args = list(seven)
        args[hole] = None
        assert bwd(B, 96, args, p) == (uns if hole == 1 else inv), hole
    assert bwd(B, Hd, seven, None) == inv and bwd(B, 96, seven, p) == uns and bwd(B, Hd, seven, off4) == inv


def test_wrapper_argument_errors():
    z = lambda *s: torch.zeros(*s)
    args = (z(3, 2, 1), z(3, 4, 1), None, z(192, 6), z(192), z(192, 64), z(192), z(64, 64))
    state = torch.zeros(2, dtype=torch.int64)
    for bad in ((state, 0, 1.0, 0.1, 0), (state, 0, 0.1, -0.1, 0), (state.float(), 0, 0.1, 0.1, 0), (state, -1, 0.1, 0.1, 0),
                (torch.zeros(3, dtype=torch.int64), 0, 0.1, 0.1, 0)):
        with pytest.raises(ValueError):
            T.decoder_step_dropout(*args, bad)


def test_a_state_off_the_launch_device_is_refused():
    """the launch dereferences ``state``: a host tensor, or one on another device than the step's, is a ValueError and never
    an address handed to a kernel -- in the wrappers, in the launch helpers themselves and in the module"""
    z = lambda *s: torch.zeros(*s)
    args = (z(3, 2, 1), z(3, 4, 1), None, z(192, 6), z(192), z(192, 64), z(192), z(64, 64))
    host = torch.zeros(2, dtype=torch.int64)
    for record in ((host, 0, 0.1, 0.1, 0), (host, 0, 0.1, 0.1), T.StepDropout(1, "cpu").take_step(0.1, 0.1)):
        with pytest.raises(ValueError, match="lives on cpu"):
            T.decoder_step_dropout(*args, record)
    enc = tools.HeightmapEncoder(2, 32, (5, 5))
    with pytest.raises(ValueError, match="lives on cpu"):
        T.decoder_step_heightmap_dropout(z(3, 3, 1), z(3, 2, 5, 5), None, enc, z(192, 35), z(192), z(192, 64), z(192), z(64, 64),
                                         (host, 0, 0.1, 0.1, 0))
    # the helpers compare with the device of their own buffers (meta tensors: nothing is dereferenced, nothing launched)
    m = lambda *s: torch.zeros(*s, device="meta")
    rec = rollout.StepDropoutRecord(host, 0, 0.1, 0.1, 0)
    with pytest.raises(ValueError, match="lives on cpu, the step's tensors on meta"):
        rollout._decoder_dropout_into(m(3, 2), m(3, 4), None, m(192, 6), m(192), m(192, 64), m(192), m(64, 64), rec, m(3, 64), m(3, 64),
                                      None, None, torch.zeros(3, 2, 1, dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError, match="lives on cpu, the step's tensors on meta"):
        rollout._decoder_hm_dropout_into(m(3, 3), m(3, 2, 5, 5), None, tuple(m(1) for _ in range(6)), m(192, 35), m(192), m(192, 64), m(192),
                                         m(64, 64), rec, m(3, 64), m(3, 64), None, None, None,
                                         torch.zeros(3, 2, 1, dtype=torch.int64, device="meta"))
    # Pointer.forward_step_dropout: device bits with a host state (``bits`` is only asked for its device before the check)
    net, enc_d, dec_s, dec_d = _net()
    net.train()
    sh, dyn, ds, dd, hh = _inputs()
    with torch.no_grad():
        proj = net.project_static(sh)
        fold = net.fold_episode(enc_d, *net.fold_decoder(dec_s, dec_d))

        class DeviceBits(object):
            is_cuda, device = True, torch.device("cuda", 0)
        with pytest.raises(ValueError, match="state lives on cpu"):
            net.forward_step_dropout(proj, DeviceBits(), fold, ds, dd, hh, T.StepDropout(1, "cpu"))
