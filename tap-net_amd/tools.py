"""Names the reference's ``tools`` module exports on the hot path (model.py:4 does ``import tools``
and builds ``tools.Container`` per env, model.py:294), backed by the HIP kernels."""
import math
import os

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from .env import BatchedContainer, Container, LockstepError, PackEngines, lockstep_containers, lockstep_scope   # noqa: F401
from .pack import reward as _reward            # noqa: F401


def calc_positions_lb_greedy(blocks, container_size, reward_type, device='cuda'):
    """tools.calc_positions_lb_greedy (tools.py:2393-2449) for one instance:
    -> positions (n, D) int, container=None (the voxel grid is never built), stable [n] bool,
    ratio = C+P+S (un-normalised), scores = [valid, box, empty, stable_num, max_h]."""
    blocks = np.asarray(blocks).astype('int')
    n, D = blocks.shape
    env = BatchedContainer(1, container_size, n, reward_type, 'full', device=device)
    for t in range(n):
        env.add_new_blocks(torch.as_tensor(blocks[t:t + 1].astype(np.int32)), want_feature=False)
    env.check()
    cnt = env.counters[0].tolist()
    hm = env.heightmap[0].cpu().numpy()
    max_h = int(hm.max())
    box = max_h * int(np.prod(container_size[:-1]))
    valid, empty, nst = cnt[0], cnt[1], cnt[2]
    ratio = (np.float64(valid) / np.float64(box) + np.float64(valid) / np.float64(empty + valid)) \
        + np.float64(nst) / np.float64(n)
    return (env.positions[0].cpu().numpy().astype(int), None, [bool(v) for v in env.stable[0].tolist()],
            float(ratio), [valid, box, empty, nst, max_h])


def is_stable_masks(bx, by, masks, use_lut=True, device='cuda'):
    """tools.is_stable (tools.py:710-765) for a batch of support patterns of one bx x by footprint that
    is off the floor: ``masks`` (n,) integers, bit (i*by + j) = footprint cell (i, j) rests on a voxel
    (tools.py:722-728).  -> (n,) bool tensor.  ``use_lut`` picks the table the 3D kernels use for
    footprints <= 4x4, False the direct form; both are the device functions the placements call."""
    dev = _lib.resolve_device(device)
    m = torch.as_tensor(np.asarray(masks, dtype=np.uint64).view(np.int64), device=dev).contiguous()
    out = torch.empty(m.numel(), dtype=torch.uint8, device=dev)
    c = _lib.ctx(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().tap_stable3d_eval(c, int(bx), int(by), _lib.ptr(m), m.numel(), 1 if use_lut else 0,
                                                _lib.ptr(out), _lib.stream_of(dev)), c)
    return out.bool()


class DqnFold(object):
    """What ``DQN.fold`` returns, the parameters of ``rollout.dqn_pick`` / ``_torch`` (tapenv.h: tap_dqn_pick has the
    algebra): the eval net with every batch-norm folded into the layer in front of it.  ``W`` columns, ``Wm`` map entries
    read, ``P`` = Wm + 2 positions, ``is_diff_height``; layer 1 per channel ``a_m``, ``b_m`` (map positions) and ``a_b``,
    ``b_b`` (block positions), ``c1`` (128, 4) their stack; ``W2`` (256, 128), ``b2``, ``W3`` (256, 256), ``b3``; ``L1``
    (512, 256 P) = lin1.weight with its columns POSITION-MAJOR, k = p * 256 + c (the reference flattens (B, 256, P)
    channel-major, c * P + p), ``l1b``; ``head_w`` (W, 512), ``head_b``.  ``W2p``, ``W3p``, ``L1p`` are W2, W3, L1 again in
    the matrix cores' operand order (``pack_mfma_operand``), what the launch streams.  Detached and contiguous, in the net's
    dtype on the net's device."""
    __slots__ = ("W", "Wm", "P", "is_diff_height", "a_m", "b_m", "a_b", "b_b", "W2", "W3", "L1") + _lib.DQN_WEIGHTS + ("_struct",)

    def weights(self, device):
        """the launch's tap_dqn_weights (built once; the record keeps the tensors it points to alive)"""
        if getattr(self, "_struct", None) is None:
            w = _lib.DqnWeights()
            w.W, w.Wm, w.P = self.W, self.Wm, self.P
            for k in _lib.DQN_WEIGHTS:
                t = getattr(self, k)
                if t.dtype != torch.float32 or t.device != torch.device(device) or not t.is_contiguous():
                    raise _lib.TapError(_lib.TAP_E_INVALID, "the fused pack-net pick takes contiguous float32 weights on %s, %s is %s on %s"
                                        % (device, k, t.dtype, t.device))
                if t.data_ptr() % 16:                                      # a view at an odd offset: the launch reads 16 bytes at a time
                    t = t.clone()
                    setattr(self, k, t)
                setattr(w, k, t.data_ptr())
            self._struct = w
        return self._struct


def pack_mfma_operand(X, T, KS):
    """X (N, K) -> (K / (4 KS), N / T, 64, 4) contiguous, the f32-input MFMA's B operand with four steps of a lane together
    (tapenv.h: tap_dqn_pick): out[q, tile, l, i] = X[tile * T + l % T, KS * (4 * q + i) + l // T]; T * KS = 64."""
    N, K = X.shape
    return X.reshape(N // T, T, K // (4 * KS), 4, KS).permute(2, 0, 4, 1, 3).reshape(K // (4 * KS), N // T, 64, 4).contiguous()


class DQN(nn.Module):
    """The learned local pack-net ("L-Pnet", tools.DQN, tools.py:3322-3367): a column for a 2D block from the
    container's height-map.  Stock PyTorch; its parameter names and shapes are the reference's, so the SL / RL
    checkpoints load with ``load_state_dict(strict=True)``.  ``output_size`` = W columns; with ``is_diff_height`` the
    map's last entry (DRL_L's trailing 0 of the 'diff' form) is dropped.  forward(height_map (B, 1, W), block (B, 1, 2))
    -> (B, W) softmax probabilities.

    ``fused`` (also an attribute; default True, what profiles/dqn_pick.json measured; no parameter, no buffer): ``pick`` -- the column and the log of its
    probability -- is ONE launch (``rollout.dqn_pick``; tapenv.h: tap_dqn_pick) when the module is in eval(), its output
    needs no gradient (grad is disabled, or neither an input nor a parameter requires one), the inputs are float32 on the
    GPU and the shape has a kernel (``rollout.dqn_pick_supported``).  In every other case ``pick`` is ``forward`` and a
    ``max``.  ``forward`` itself is always the torch path."""

    def __init__(self, output_size, is_diff_height, fused=True):
        super(DQN, self).__init__()
        self.fused = bool(fused)
        self._fold = None
        self.conv_height_map = nn.Conv1d(1, 128, kernel_size=1)
        self.conv_block = nn.Conv1d(1, 128, kernel_size=1)
        self.bn1 = nn.BatchNorm1d(128)
        self.conv2 = nn.Conv1d(128, 256, kernel_size=1)
        self.bn2 = nn.BatchNorm1d(256)
        self.conv3 = nn.Conv1d(256, 256, kernel_size=1)
        self.bn3 = nn.BatchNorm1d(256)
        # positions along the conv axis: the map (W, or W - 1 with the diff input) and the block's two sides --
        # 1 536 / 1 792 inputs for the reference's W = 5
        self.lin1 = nn.Linear(256 * (output_size - (1 if is_diff_height else 0) + 2), 512)
        self.head = nn.Linear(512, output_size)
        self.is_diff_height = is_diff_height

    def forward(self, height_map, block):
        if self.is_diff_height:
            height_map = height_map[:, :, :-1]
        h = torch.cat((self.conv_height_map(height_map), self.conv_block(block)), dim=-1)
        h = F.relu(self.bn1(h))
        h = F.relu(self.bn2(self.conv2(h)))
        h = F.relu(self.bn3(self.conv3(h)))
        h = F.relu(self.lin1(h.reshape(h.size(0), -1)))
        return F.softmax(self.head(h), dim=1)

    def fold(self):
        """-> a ``DqnFold``: the eval net, each batch-norm (its running statistics and its own eps) folded into the layer in
        front of it, in torch, in the parameters' dtype (``net.double().fold()`` is the float64 model), detached; no
        parameter is added and the state-dict keys stay the reference's.  Valid in eval() only.  The record is kept until a
        parameter or a running statistic changes (its version, memory or dtype); one computed under hipGraph capture is
        not kept."""
        if self.training:
            raise RuntimeError("DQN.fold folds the running statistics: the net must be in eval()")
        tensors = list(self.parameters()) + list(self.buffers())
        key = tuple((t.data_ptr(), t._version, t.dtype) for t in tensors) + tuple(bn.eps for bn in (self.bn1, self.bn2, self.bn3))
        if self._fold is not None and self._fold[0] == key:
            return self._fold[1]
        with torch.no_grad():
            f = DqnFold()
            f.W, f.is_diff_height = int(self.head.out_features), bool(self.is_diff_height)
            f.P = int(self.lin1.in_features) // 256
            f.Wm = f.P - 2

            def scale(bn):
                return bn.weight / torch.sqrt(bn.running_var + bn.eps)
            s1, s2, s3 = scale(self.bn1), scale(self.bn2), scale(self.bn3)
            f.a_m = s1 * self.conv_height_map.weight[:, 0, 0]
            f.b_m = s1 * (self.conv_height_map.bias - self.bn1.running_mean) + self.bn1.bias
            f.a_b = s1 * self.conv_block.weight[:, 0, 0]
            f.b_b = s1 * (self.conv_block.bias - self.bn1.running_mean) + self.bn1.bias
            f.c1 = torch.stack((f.a_m, f.b_m, f.a_b, f.b_b), 1)
            f.W2 = s2[:, None] * self.conv2.weight[:, :, 0]
            f.b2 = s2 * (self.conv2.bias - self.bn2.running_mean) + self.bn2.bias
            f.W3 = s3[:, None] * self.conv3.weight[:, :, 0]
            f.b3 = s3 * (self.conv3.bias - self.bn3.running_mean) + self.bn3.bias
            f.L1 = self.lin1.weight.reshape(512, 256, f.P).transpose(1, 2).reshape(512, 256 * f.P)   # c * P + p -> p * 256 + c
            f.l1b, f.head_w, f.head_b = self.lin1.bias, self.head.weight, self.head.bias
            f.W2p, f.W3p, f.L1p = pack_mfma_operand(f.W2, 32, 2), pack_mfma_operand(f.W3, 32, 2), pack_mfma_operand(f.L1, 16, 4)
            for k in ("a_m", "b_m", "a_b", "b_b", "W2", "W3", "L1") + _lib.DQN_WEIGHTS:
                setattr(f, k, getattr(f, k).detach().contiguous())
        if not (tensors and tensors[0].is_cuda and torch.cuda.is_current_stream_capturing()):
            self._fold = (key, f)
        return f

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_fold'] = None                   # a cache holding device addresses: a copy folds again
        return state

    def _takes_launch(self, height_map, block):
        """whether this pick is the one launch (the class docstring has the conditions)"""
        if not getattr(self, 'fused', False) or self.training:
            return False
        if not (height_map.is_cuda and block.is_cuda and height_map.dtype == torch.float32 and block.dtype == torch.float32):
            return False
        if torch.is_grad_enabled() and (height_map.requires_grad or block.requires_grad or
                                        any(p.requires_grad for p in self.parameters())):
            return False
        from .rollout import dqn_pick_supported
        return self.lin1.weight.dtype == torch.float32 and self.lin1.weight.device == height_map.device and \
            dqn_pick_supported(self.head.out_features, self.is_diff_height)

    def pick(self, height_map, block):
        """height_map (B, 1, W), block (B, 1, 2) -> x (B,) int64, the first column of the largest probability, and logp (B,),
        the log of that probability (model.py:1200-1202): one launch under ``fused`` (the class docstring has the
        conditions), else ``forward(...).max(1)`` and ``.log()``."""
        if self._takes_launch(height_map, block):
            from .rollout import dqn_pick
            return dqn_pick(self.fold(), height_map, block)
        best = self.forward(height_map, block).max(1)
        return best[1], best[0].log()


class DynamicBitsEncoder(nn.Module):
    """The reference actor's ``dynamic_encoder`` (model.py:380; an Encoder whose only layer is ``conv``, a
    Conv1d(rows, hidden_size, kernel_size=1)) with a second input form: its state dict -- ``conv.weight``,
    ``conv.bias`` -- loads with ``strict=True``.  ``forward(x)``: an int64 tensor is the bit shadow of ``dynamic``
    (``EpisodeStepper.dynamic_bits``, ``pack.dynamic_bits``) and goes through ``rollout.encode_dynamic_bits`` -- one
    launch, no fp32 ``dynamic`` anywhere, the shadow kept for the backward --; a floating tensor is the fp32 ``dynamic``
    (B, rows, nR) and goes through ``F.conv1d``, so the module can replace the reference's encoder before a trainer
    moves to ``EpisodeStepper(expand_dynamic=False)``."""

    def __init__(self, rows, hidden_size):
        super(DynamicBitsEncoder, self).__init__()
        self.rows, self.hidden_size = int(rows), int(hidden_size)
        self.conv = nn.Conv1d(self.rows, self.hidden_size, kernel_size=1)

    def forward(self, x):
        if x.dtype is torch.int64:
            from .rollout import encode_dynamic_bits
            return encode_dynamic_bits(x, self.conv.weight, self.conv.bias, rows=self.rows)
        if not x.is_floating_point():
            raise TypeError("DynamicBitsEncoder takes the int64 shadow or the floating `dynamic`, got %s" % (x.dtype,))
        return F.conv1d(x, self.conv.weight, self.conv.bias)


class HeightmapEncoder(nn.Module):
    """The reference's 3D ``dynamic_decoder`` (model.py:21-35) with its constructor and its children ``conv1``, ``conv2``,
    ``conv3`` only: a checkpoint's ``dynamic_decoder.*`` loads with ``strict=True``.  ``hidden_size`` = m; conv1
    (m / 4, input_size, 1, 1) and conv2 (m / 2, m / 4, 1, 1) have stride 2, conv3 (m, m / 2, ceil(W / 4), ceil(L / 4)) covers
    what is left of the map, so ``forward(hm (B, input_size, W, L))`` -> (B, m, 1) reads the cells (4i, 4j) only.  ``forward``
    is the reference's arithmetic in torch, any dtype and device; on the device the encoder runs inside the decoder step's
    launch (``rollout.decoder_step_heightmap``, ``Pointer.fold_decoder(dynamic_decoder=<HeightmapEncoder>)``)."""

    def __init__(self, input_size, hidden_size, map_size):
        super(HeightmapEncoder, self).__init__()
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.map_size = (int(map_size[0]), int(map_size[1]))
        self.conv1 = nn.Conv2d(input_size, int(hidden_size / 4), stride=2, kernel_size=1)
        self.conv2 = nn.Conv2d(int(hidden_size / 4), int(hidden_size / 2), stride=2, kernel_size=1)
        self.conv3 = nn.Conv2d(int(hidden_size / 2), int(hidden_size),
                               kernel_size=(math.ceil(map_size[0] / 4), math.ceil(map_size[1] / 4)))

    def forward(self, input):
        output = F.leaky_relu(self.conv1(input))
        output = F.leaky_relu(self.conv2(output))
        return self.conv3(output).squeeze(-1)


def _is_heightmap_encoder(enc):
    """a HeightmapEncoder, or anything with conv1 .. conv3 whose weights have four axes"""
    return all(getattr(getattr(enc, name, None), "weight", None) is not None and getattr(enc, name).weight.dim() == 4
               for name in ("conv1", "conv2", "conv3"))


class _Attention(nn.Module):
    """The reference's Attention (model.py:38-74) as a parameter holder: ``v`` (1, 1, Hd) and ``W`` (1, Hd, 2 He + Hd),
    columns [static | dynamic | decoder]; Pointer.forward does its arithmetic."""

    def __init__(self, encoder_hidden_size, decoder_hidden_size):
        super(_Attention, self).__init__()
        self.v = nn.Parameter(torch.zeros((1, 1, decoder_hidden_size), requires_grad=True))
        self.W = nn.Parameter(torch.zeros((1, decoder_hidden_size, 2 * encoder_hidden_size + decoder_hidden_size),
                                          requires_grad=True))


class Pointer(nn.Module):
    """The reference actor's ``pointer`` (model.py:77-138; its Attention, model.py:38-74) with a second input form.  The
    constructor is the reference's and so are the parameter names and shapes -- ``W`` (1, Hd, 4 He), ``v`` (1, 1, Hd),
    ``encoder_attn.W`` (1, Hd, 2 He + Hd), ``encoder_attn.v``, ``gru.*`` --: a reference checkpoint's ``pointer.*`` loads
    with ``strict=True``.  He / Hd are ``encoder_hidden_size`` / ``decoder_hidden_size``.

    ``forward(static_hidden, dynamic_hidden, decoder_hidden, last_hh)`` -> (probs (B, nR), last_hh): the reference's
    arithmetic in torch, any dtype and device.

    ``project_static(static_hidden)`` -> proj (B, 3, nR, Hd), once per episode, differentiable: what the two W do to
    static_hidden, in ``rollout.pointer_scores``' layout.  ``forward_bits(proj, bits, dynamic_encoder, decoder_hidden,
    last_hh)`` -> (logits, last_hh): the GRU step and both dropouts in torch exactly as ``forward`` runs them, the
    dynamic encoder's ``conv`` folded into the two W under autograd (M, k), q from the GRU's output, then ONE launch from
    the int64 shadow ``bits`` (a stepper's ``dynamic_bits``) to the logits: no dynamic_hidden, no concatenation.  On a
    shape without a kernel ``forward_bits`` runs ``forward`` on ``dynamic_encoder(bits)`` and the static_hidden that
    ``project_static`` was given (the returned tensor carries it as ``proj.static_hidden``).

    ``fold_decoder(...)`` -> (P, c) and ``fold_episode(dynamic_encoder, P, c)`` -> fold, once per episode, differentiable:
    the decoder's 1x1 encoders folded into the GRU's input weights, and everything else of a step that depends on the
    parameters alone (M, k, Wq).  ``forward_step(proj, bits, fold, decoder_static, decoder_dynamic, last_hh)`` -> (logits,
    last_hh) is then TWO launches: ``rollout.decoder_step`` (input product, GRU cell and q; with a ``HeightmapEncoder`` as the
    dynamic decoder ``rollout.decoder_step_heightmap``, which runs that encoder too) and ``rollout.pointer_scores``.

    ``forward_step_dropout(..., last_hh, dropout)`` and ``forward_bits_dropout(..., last_hh, dropout)`` are the training
    forms: ``dropout`` is a ``StepDropout``, whose counter-based masks replace torch's generator -- inside the first launch
    where there is one, through ``rollout.dropout_keep_words`` on the torch path.

    ``fold_static(static_encoder, static_input)`` -> ``StaticFold``, once per episode, differentiable in the encoder's and the
    two W's parameters: the static encoder folded into the two W (G, g) beside the rows ``xs`` of ``static`` it sees.  The
    record is accepted wherever ``proj`` is -- ``forward_bits``, ``forward_step`` and both ``_dropout`` forms --; the pointer
    launch is then ``rollout.pointer_scores_static``, which computes the static term from ``xs`` inside the launch: an episode
    has no static_hidden and no ``proj``.  The dispatch is on the type: a tensor goes the way described above.  With the
    record the torch path is ``forward`` on ``static_encoder(xs)``, in the dtype it is given, and is taken off the GPU, on a
    shape without a kernel and, in ``forward_step``, under the conditions listed there."""

    def __init__(self, encoder_hidden_size, decoder_hidden_size, decoder_input_type, input_type, num_layers=1, dropout=0.2):
        super(Pointer, self).__init__()
        self.encoder_hidden_size = encoder_hidden_size
        self.decoder_hidden_size = decoder_hidden_size
        self.num_layers = num_layers
        self.decoder_input_type = decoder_input_type
        self.input_type = input_type
        self.v = nn.Parameter(torch.zeros((1, 1, decoder_hidden_size), requires_grad=True))
        self.W = nn.Parameter(torch.zeros((1, decoder_hidden_size, 4 * encoder_hidden_size), requires_grad=True))
        self.gru = nn.GRU(decoder_hidden_size, decoder_hidden_size, num_layers, batch_first=True,
                          dropout=dropout if num_layers > 1 else 0)
        self.encoder_attn = _Attention(encoder_hidden_size, decoder_hidden_size)
        self.drop_rnn = nn.Dropout(p=dropout)
        self.drop_hh = nn.Dropout(p=dropout)

    def _gru_step(self, decoder_hidden, last_hh, keep=None):
        """model.py:108-115: the GRU step and the two dropouts -> rnn_out (B, Hd), last_hh.  ``keep``: packed keep words
        (B, 2, Hd / 64) int64 (``rollout.dropout_keep_words``) -- those masks are applied instead of ``drop_rnn`` / ``drop_hh``:
        a kept element is x s with s = float32(1 / (1 - p)), a dropped one 0, in the dtype of x.  With one layer torch's
        generator is not touched; with more, ``nn.GRU``'s own inter-layer dropout still draws from it, and plane 1 is unused
        (``drop_hh`` is not applied there, as without ``keep``)."""
        rnn_out, last_hh = self.gru(decoder_hidden.transpose(2, 1), last_hh)
        rnn_out = rnn_out.squeeze(1)
        if keep is None:
            rnn_out = self.drop_rnn(rnn_out)
            if self.num_layers == 1:
                last_hh = self.drop_hh(last_hh)     # with more layers the GRU has applied it
            return rnn_out, last_hh
        from .rollout import dropout_keep_mask, dropout_scale

        def masked(x, kept, p):
            return torch.zeros_like(x) if p >= 1 else torch.where(kept, x * dropout_scale(p), torch.zeros_like(x))
        mask = dropout_keep_mask(keep.to(rnn_out.device))
        rnn_out = masked(rnn_out, mask[:, 0], self.drop_rnn.p)
        if self.num_layers == 1:
            last_hh = masked(last_hh, mask[:, 1].unsqueeze(0), self.drop_hh.p)
        return rnn_out, last_hh

    def _step_dropout(self, dropout):
        """-> the record of the next step of a ``StepDropout`` (or the record itself, when ``forward_step`` has taken it) in
        training mode, else None: in ``eval()`` the keyword is ignored and the step counter stays where it is"""
        if dropout is None or not self.training:
            return None
        return dropout.take_step(self.drop_rnn.p, self.drop_hh.p) if hasattr(dropout, "take_step") else dropout

    def _keep_words(self, rec, B):
        """the torch path's masks for a record: the same words the dropout launch would write"""
        from .rollout import dropout_keep_words
        return None if rec is None else dropout_keep_words(rec.state, rec.step, B, self.decoder_hidden_size, rec.p_rnn, rec.p_hh,
                                                           rec.env_offset)

    def forward(self, static_hidden, dynamic_hidden, decoder_hidden, last_hh):
        return self._forward(static_hidden, dynamic_hidden, decoder_hidden, last_hh)

    def _forward(self, static_hidden, dynamic_hidden, decoder_hidden, last_hh, keep=None):
        rnn_out, last_hh = self._gru_step(decoder_hidden, last_hh, keep)
        B, nR = static_hidden.size(0), static_hidden.shape[-1]
        encoder_hidden = torch.cat((static_hidden, dynamic_hidden), 1)
        # Attention.forward (model.py:55-74)
        hidden = torch.cat((encoder_hidden, rnn_out.unsqueeze(2).repeat(1, 1, nR)), 1)
        at = self.encoder_attn
        attns = torch.bmm(at.v.expand(B, 1, -1), torch.tanh(torch.bmm(at.W.expand(B, -1, -1), hidden)))
        enc_attn = F.softmax(attns, dim=2)
        context = enc_attn.bmm(encoder_hidden.permute(0, 2, 1))                       # (B, 1, 2 He)
        context = context.transpose(1, 2).expand_as(encoder_hidden)
        energy = torch.cat((encoder_hidden, context), dim=1)
        probs = torch.bmm(self.v.expand(B, -1, -1), torch.tanh(torch.bmm(self.W.expand(B, -1, -1), energy))).squeeze(1)
        return probs, last_hh

    def folded_weights(self):
        """-> Ws, Wd (3 Hd, He): the columns of the two W that meet static_hidden / dynamic_hidden, stacked as the
        attention's, the pointer's and the context's segment; Wq (Hd, Hd): the attention's columns for the decoder"""
        He = self.encoder_hidden_size
        Wa, Wp = self.encoder_attn.W[0], self.W[0]
        Ws = torch.cat((Wa[:, :He], Wp[:, :He], Wp[:, 2 * He:3 * He]), 0)
        Wd = torch.cat((Wa[:, He:2 * He], Wp[:, He:2 * He], Wp[:, 3 * He:4 * He]), 0)
        return Ws, Wd, Wa[:, 2 * He:]

    def project_static(self, static_hidden):
        Ws = self.folded_weights()[0]
        B, He, nR = static_hidden.shape
        proj = torch.matmul(static_hidden.transpose(1, 2), Ws.t().to(static_hidden.dtype))       # (B, nR, 3 Hd)
        proj = proj.view(B, nR, 3, self.decoder_hidden_size).permute(0, 2, 1, 3).contiguous()
        proj.static_hidden = static_hidden
        return proj

    def fold_static(self, static_encoder, static_input):
        """-> the ``StaticFold`` that stands where ``proj`` stands, once per episode: static_hidden = Es . xs + bs is a 1x1
        convolution of the S rows ``static_input`` (B, S, nR) of ``static`` that the encoder sees (the reference's
        ``static[:, 1:, :]``), so proj = g + G . xs with G = Ws . Es (3 Hd, S) and g = Ws . bs (3 Hd,), Ws from
        ``folded_weights``.  G and g are differentiable in the encoder's and the two W's parameters; ``xs`` is kept detached
        and contiguous.  ``static_encoder``: anything with a kernel-size-1 ``.conv``, or an ``nn.Conv1d`` itself."""
        conv = getattr(static_encoder, "conv", static_encoder)
        w = conv.weight
        if w.dim() != 3 or int(w.shape[2]) != 1:
            raise ValueError("the static encoder must be a kernel-size-1 convolution, got a weight of shape %s" % (tuple(w.shape),))
        if static_input.dim() != 3 or int(static_input.shape[1]) != int(w.shape[1]) or not static_input.is_floating_point():
            raise ValueError("static_input must be a floating (B, %d, nR) tensor, got %s %s"
                             % (int(w.shape[1]), static_input.dtype, tuple(static_input.shape)))
        Ws = self.folded_weights()[0]
        sf = StaticFold()
        sf.static_encoder = static_encoder
        sf.xs = static_input.detach().contiguous()
        sf.G = Ws.matmul(w[:, :, 0].to(Ws.dtype))
        sf.g = Ws.matmul(conv.bias.to(Ws.dtype)) if conv.bias is not None else torch.zeros_like(Ws[:, 0])
        sf.S, sf.nR = int(static_input.shape[1]), int(static_input.shape[2])
        return sf

    def _forward_static_torch(self, sf, bits, dynamic_encoder, decoder_hidden, last_hh, keep):
        """the torch path of a step whose static side is a ``StaticFold``: ``forward`` on ``static_encoder(xs)`` and the
        dynamic encoder's output.  A shadow off the GPU is unpacked to the 0/1 ``dynamic``; anything else goes to the encoder
        as it is"""
        conv = dynamic_encoder.conv
        if bits.dtype is torch.int64 and not bits.is_cuda:
            rows = int(conv.weight.shape[1])
            w = bits.reshape(bits.shape[0], 2 if rows > 64 else 1, sf.nR)
            r = torch.arange(rows, device=bits.device)
            dynamic_hidden = dynamic_encoder(((w[:, r // 64, :] >> (r % 64).view(1, rows, 1)) & 1).to(conv.weight.dtype))
        else:
            dynamic_hidden = dynamic_encoder(bits)
        return self._forward(sf.static_encoder(sf.xs), dynamic_hidden, decoder_hidden, last_hh, keep)

    def forward_bits(self, proj, bits, dynamic_encoder, decoder_hidden, last_hh):
        return self._forward_bits(proj, bits, dynamic_encoder, decoder_hidden, last_hh, None)

    def forward_bits_dropout(self, proj, bits, dynamic_encoder, decoder_hidden, last_hh, dropout):
        """``forward_bits`` with a ``StepDropout`` as the random source: in training mode the GRU step takes the masks of its
        next record (``rollout.dropout_keep_words``) instead of torch's generator -- the masks ``forward_step_dropout``'s
        launch applies for the same (state, step).  In ``eval()`` it is ``forward_bits`` and the step counter stays."""
        return self._forward_bits(proj, bits, dynamic_encoder, decoder_hidden, last_hh, dropout)

    def _forward_bits(self, proj, bits, dynamic_encoder, decoder_hidden, last_hh, dropout, torch_only=False):
        from .rollout import pointer_scores, pointer_scores_static, pointer_scores_static_supported, pointer_scores_supported
        conv = dynamic_encoder.conv
        static = isinstance(proj, StaticFold)
        rows, nR, Hd = int(conv.weight.shape[1]), proj.nR if static else int(proj.shape[2]), self.decoder_hidden_size
        keep = self._keep_words(self._step_dropout(dropout), int(decoder_hidden.shape[0]))
        if static:
            if torch_only or not bits.is_cuda or bits.dtype is not torch.int64 or not pointer_scores_static_supported(rows, nR, Hd, proj.S):
                return self._forward_static_torch(proj, bits, dynamic_encoder, decoder_hidden, last_hh, keep)
            rnn_out, last_hh = self._gru_step(decoder_hidden, last_hh, keep)
            _, Wd, Wq = self.folded_weights()
            M = Wd.matmul(conv.weight[:, :, 0])
            k = Wd.matmul(conv.bias) if conv.bias is not None else torch.zeros_like(Wd[:, 0])
            q = rnn_out.matmul(Wq.t())
            return pointer_scores_static(proj.xs, bits, proj.G, proj.g, M, k, q, self.encoder_attn.v[0, 0], self.v[0, 0], rows=rows), last_hh
        if not pointer_scores_supported(rows, nR, Hd):
            static_hidden = getattr(proj, "static_hidden", None)
            if static_hidden is None:
                raise ValueError("no pointer kernel for rows %d, nR %d, Hd %d, and proj does not come from project_static: "
                                 "call forward(static_hidden, dynamic_encoder(bits), ...)" % (rows, nR, Hd))
            return self._forward(static_hidden, dynamic_encoder(bits), decoder_hidden, last_hh, keep)
        rnn_out, last_hh = self._gru_step(decoder_hidden, last_hh, keep)
        _, Wd, Wq = self.folded_weights()
        M = Wd.matmul(conv.weight[:, :, 0])
        k = Wd.matmul(conv.bias) if conv.bias is not None else torch.zeros_like(Wd[:, 0])
        q = rnn_out.matmul(Wq.t())
        return pointer_scores(proj, bits, M, k, q, self.encoder_attn.v[0, 0], self.v[0, 0], rows=rows), last_hh

    def fold_decoder(self, static_decoder=None, dynamic_decoder=None, combine='cat', identity_dynamic=0):
        """-> P (3 Hd, K), c (3 Hd,): the decoder's encoders (model.py:218-221, 352-354) folded into the GRU's input weights,
        differentiable, once per episode: gi = weight_ih_l0 . decoder_hidden + bias_ih_l0 = P . [xs ; xd] + c.  An encoder
        is anything with a kernel-size-1 ``.conv`` (the reference's Encoder, ``DynamicBitsEncoder``) or an ``nn.Conv1d``
        itself; either may be None.  ``combine='cat'``: decoder_hidden = cat(static(xs), dynamic(xd)), the encoders' rows
        adding up to Hd; ``'sum'``: static(xs) + dynamic(xd), Hd rows each.  ``identity_dynamic=m`` (instead of a dynamic
        encoder): the caller passes an already encoded dynamic half of m rows as xd, and the fold takes m identity columns
        for it.  A ``HeightmapEncoder`` as ``dynamic_decoder`` (the reference's 3D one; anything with four-axis ``conv1`` ..
        ``conv3``) has leaky-ReLUs and does not fold: the fold takes m = its hidden size identity columns and no bias for that
        half -- conv3's bias lives in the encoder's output --, and the encoder itself runs inside the step's launch
        (``rollout.decoder_step_heightmap``).  K = the static encoder's inputs + the dynamic encoder's inputs (or m).  P
        carries what ``forward_step`` needs (``P.static_decoder``, ``P.dynamic_decoder``, ``P.combine``,
        ``P.identity_dynamic``)."""
        if combine not in ('cat', 'sum'):
            raise ValueError("combine must be 'cat' or 'sum', not %r" % (combine,))
        m = int(identity_dynamic)
        if m < 0 or (m and dynamic_decoder is not None):
            raise ValueError("identity_dynamic stands in for the dynamic encoder: pass one of them")
        if static_decoder is None and dynamic_decoder is None and not m:
            raise ValueError("fold_decoder needs at least one encoder")
        Hd = self.decoder_hidden_size
        W_ih = self.gru.weight_ih_l0
        heightmap = dynamic_decoder is not None and _is_heightmap_encoder(dynamic_decoder)
        parts = []                                      # (weight (rows, inputs), bias (rows,)) of each half of decoder_hidden
        for enc in (static_decoder, None if heightmap else dynamic_decoder):
            if enc is None:
                continue
            conv = getattr(enc, "conv", enc)
            w = conv.weight
            if w.dim() != 3 or int(w.shape[2]) != 1:
                raise ValueError("a decoder encoder must be a kernel-size-1 convolution, got a weight of shape %s" % (tuple(w.shape),))
            w = w[:, :, 0].to(W_ih.dtype)
            parts.append((w, conv.bias.to(W_ih.dtype) if conv.bias is not None else torch.zeros_like(w[:, 0])))
        mi = int(dynamic_decoder.conv3.weight.shape[0]) if heightmap else m
        if mi:
            parts.append((torch.eye(mi, dtype=W_ih.dtype, device=W_ih.device), torch.zeros(mi, dtype=W_ih.dtype, device=W_ih.device)))
        widths = [int(w.shape[0]) for w, _ in parts]
        if (sum(widths) != Hd) if combine == 'cat' else any(v != Hd for v in widths):
            raise ValueError("the encoders give %s rows; the GRU takes %d (combine=%r)" % (widths, Hd, combine))
        if combine == 'cat':
            cuts = [sum(widths[:i]) for i in range(len(widths) + 1)]
            P = torch.cat([W_ih[:, cuts[i]:cuts[i + 1]].matmul(w) for i, (w, _) in enumerate(parts)], dim=1)
            c = W_ih.matmul(torch.cat([b for _, b in parts]))
        else:
            P = torch.cat([W_ih.matmul(w) for w, _ in parts], dim=1)
            c = W_ih.matmul(sum(b for _, b in parts))
        if self.gru.bias:
            c = c + self.gru.bias_ih_l0
        P.static_decoder, P.dynamic_decoder, P.combine, P.identity_dynamic = static_decoder, dynamic_decoder, combine, m
        return P, c

    def fold_episode(self, dynamic_encoder, P, c):
        """-> the record ``forward_step`` takes, once per episode, differentiable: everything of a step that depends on the
        parameters alone -- M, k (the dynamic encoder folded into the two W, as ``forward_bits`` folds it per step), P, c
        (``fold_decoder``), Wq (the attention's columns for the decoder, contiguous), the two v and the GRU's four tensors."""
        conv = dynamic_encoder.conv
        _, Wd, Wq = self.folded_weights()
        fold = StepFold()
        fold.dynamic_encoder, fold.rows = dynamic_encoder, int(conv.weight.shape[1])
        fold.M = Wd.matmul(conv.weight[:, :, 0])
        fold.k = Wd.matmul(conv.bias) if conv.bias is not None else torch.zeros_like(Wd[:, 0])
        fold.P, fold.c, fold.Wq = P, c, Wq.contiguous()
        fold.va, fold.vp = self.encoder_attn.v[0, 0], self.v[0, 0]
        fold.w_ih, fold.w_hh = self.gru.weight_ih_l0, self.gru.weight_hh_l0
        fold.b_ih, fold.b_hh = (self.gru.bias_ih_l0, self.gru.bias_hh_l0) if self.gru.bias else (None, None)
        fold.static_decoder, fold.dynamic_decoder = getattr(P, "static_decoder", None), getattr(P, "dynamic_decoder", None)
        fold.combine, fold.identity_dynamic = getattr(P, "combine", None), getattr(P, "identity_dynamic", 0)
        fold.heightmap = fold.dynamic_decoder if fold.dynamic_decoder is not None and _is_heightmap_encoder(fold.dynamic_decoder) else None
        return fold

    def _decoder_hidden(self, fold, decoder_static, decoder_dynamic):
        """the unfolded decoder_hidden (B, Hd, 1) of model.py:352-354 from the encoders ``fold_decoder`` was given"""
        if fold.combine is None:
            raise ValueError("fold.P does not come from fold_decoder: the torch path needs the decoder's encoders")
        B = int((decoder_static if decoder_static is not None else decoder_dynamic).shape[0])
        halves = []
        if fold.static_decoder is not None:
            halves.append(fold.static_decoder(decoder_static.reshape(B, -1, 1)))
        if fold.heightmap is not None:
            halves.append(fold.heightmap(decoder_dynamic))      # (B, C, W, L) as the stepper hands it out -> (B, m, 1)
        elif fold.dynamic_decoder is not None:
            halves.append(fold.dynamic_decoder(decoder_dynamic.reshape(B, -1, 1)))
        elif fold.identity_dynamic:
            halves.append(decoder_dynamic.reshape(B, -1, 1))
        return torch.cat(halves, dim=1) if fold.combine == 'cat' else sum(halves)

    def forward_step(self, proj, bits, fold, decoder_static, decoder_dynamic, last_hh):
        """A decoding step in TWO launches -> (logits (B, nR), last_hh (1, B, Hd)): ``rollout.decoder_step`` from the stepper's
        ``decoder_static`` / ``decoder_dynamic`` and ``last_hh`` (the reference's (1, B, Hd), or None for zeros) to the new
        hidden state and q, then ``rollout.pointer_scores`` from the shadow ``bits`` to the logits.  ``proj`` from
        ``project_static``, ``fold`` from ``fold_episode`` (both once per episode).  Either input may be None when
        ``fold_decoder`` had no encoder for it.  With a ``HeightmapEncoder`` as the fold's dynamic decoder (a 3D actor) the first
        launch is ``rollout.decoder_step_heightmap`` -- the encoder runs inside it -- and ``decoder_dynamic`` is the stepper's 4-D
        (B, C, W, L) feature, which the torch path hands to the encoder as it is.  The torch path -- ``_gru_step`` on the unfolded decoder_hidden, then what
        ``forward_bits`` does: today's result -- runs instead when dropout would be active (training with p > 0), with more
        than one GRU layer, with a GRU without bias, off the GPU, or on a shape without a kernel for either launch.
        ``forward_step_dropout`` keeps a training step with dropout on the two launches."""
        return self._forward_step(proj, bits, fold, decoder_static, decoder_dynamic, last_hh, None)

    def forward_step_dropout(self, proj, bits, fold, decoder_static, decoder_dynamic, last_hh, dropout):
        """``forward_step`` for training with dropout: ``dropout`` is a ``StepDropout``.  In training mode the step takes its
        next record; ``drop_rnn.p`` / ``drop_hh.p`` are read at the call, and the two masks run INSIDE the first launch
        (``rollout.decoder_step_dropout`` / ``decoder_step_heightmap_dropout``): last_hh = drop_hh(h'), q from drop_rnn(h').
        Wherever the torch path is still taken -- off the GPU, several GRU layers, a GRU without bias, a shape without a kernel,
        p = 1 -- it applies ``rollout.dropout_keep_words`` for the same record, so both paths are the same function of the same
        masks, and with one GRU layer torch's generator is never touched.  With ``num_layers > 1`` only ``drop_rnn`` takes the
        record's mask: ``nn.GRU`` applies its own dropout between the layers and to nothing after the last, from torch's
        generator, and ``drop_hh`` is not applied, as in ``forward``.  A ``StepDropout`` whose state is not on the device of
        ``bits`` raises ValueError.  In ``eval()`` it is ``forward_step`` and the step counter stays."""
        return self._forward_step(proj, bits, fold, decoder_static, decoder_dynamic, last_hh, dropout)

    def forward_step_pick(self, static_fold, bits, fold, decoder_static, decoder_dynamic, last_hh, current_mask, source=None,
                          dropout=None, want_logits=False):
        """An INFERENCE step with its pick in TWO launches -> (ptr (B,) int64, logp (B,) float32[, logits], last_hh): the decoder
        step as ``forward_step`` / ``forward_step_dropout`` chooses it (plain, height-map, dropout -- ``dropout`` is a
        ``StepDropout``, read in training mode only), then ``rollout.pointer_pick_static``: scores and pick in one launch, the
        logits never leaving it, ``static_fold.xs`` read as the view it is (``StaticFold.with_rows``).  ``current_mask``: the
        stepper's; ``source`` None picks greedily, a ``StepDropout`` / ``PickRecord`` draws.  ``want_logits`` returns the
        logits too (the launch stores them as ``pointer_scores_static`` does).  The bytes are those of ``forward_step[_dropout]``
        followed by ``rollout.pointer_pick`` / ``pointer_pick_draw``, and exactly those launches run instead -- ``pointer_pick_torch``
        off the GPU -- when grad is enabled and something requires it, off the GPU, on a shape without a kernel, wherever
        ``forward_step`` takes its torch path, and when ``static_fold`` is a ``proj`` tensor."""
        from .rollout import _pick_record, pick_uniforms, pointer_pick, pointer_pick_draw, pointer_pick_torch
        out = self._forward_step(static_fold, bits, fold, decoder_static, decoder_dynamic, last_hh, dropout,
                                 pick=(current_mask, source, want_logits))
        if len(out) > 2:
            return out
        logits, last_hh = out
        if not logits.is_cuda:
            u = None
            if source is not None:
                rec = _pick_record(source)
                u = pick_uniforms(rec.state, rec.step, int(logits.shape[0]), rec.env_offset)
            ptr, logp = pointer_pick_torch(logits, current_mask, u)
        elif source is not None:
            ptr, logp = pointer_pick_draw(logits, current_mask, source)
        else:
            ptr, logp = pointer_pick(logits, current_mask)
        return (ptr, logp, logits, last_hh) if want_logits else (ptr, logp, last_hh)

    def _forward_step(self, proj, bits, fold, decoder_static, decoder_dynamic, last_hh, dropout, pick=None):
        from .rollout import (decoder_step_heightmap_supported, decoder_step_supported, pointer_pick_static, pointer_scores,
                              pointer_scores_static, pointer_scores_static_supported, pointer_scores_supported, _decoder_step,
                              _decoder_step_heightmap)
        static = isinstance(proj, StaticFold)
        Hd, nR = self.decoder_hidden_size, proj.nR if static else int(proj.shape[2])
        Ks = 0 if decoder_static is None or fold.static_decoder is None else int(decoder_static[0].numel())
        Kd = 0 if decoder_dynamic is None or (fold.dynamic_decoder is None and not fold.identity_dynamic) else int(decoder_dynamic[0].numel())
        rec = self._step_dropout(dropout)
        if rec is not None and bits.is_cuda and rec.state.device != bits.device:
            # the launch would dereference the state on its own device; a copy would cut a captured graph off from it
            raise ValueError("the StepDropout's state lives on %s, the step's tensors on %s: build it with StepDropout(seed, %r)"
                             % (rec.state.device, bits.device, str(bits.device)))
        # without a record active dropout is torch's own and stays on the torch path; with one only p = 1 does
        dropping = self.training and ((self.drop_rnn.p > 0 or self.drop_hh.p > 0) if rec is None else max(rec.p_rnn, rec.p_hh) >= 1)
        hm = fold.heightmap
        if hm is not None:
            m = int(hm.conv3.weight.shape[0])
            launch = decoder_dynamic is not None and decoder_dynamic.dim() == 4 and Ks + m == int(fold.P.shape[1]) and \
                int(hm.conv1.weight.shape[1]) == int(decoder_dynamic.shape[1]) and \
                tuple(hm.conv3.weight.shape[2:]) == tuple((int(v) + 3) // 4 for v in decoder_dynamic.shape[2:]) and \
                decoder_step_heightmap_supported(Ks, *decoder_dynamic.shape[1:], m, Hd)
        else:
            launch = Ks + Kd == int(fold.P.shape[1]) and decoder_step_supported(Ks, Kd, Hd)
        kernel = pointer_scores_static_supported(fold.rows, nR, Hd, proj.S) and bits.dtype is torch.int64 if static else \
            pointer_scores_supported(fold.rows, nR, Hd)
        if dropping or self.num_layers != 1 or not self.gru.bias or not bits.is_cuda or not launch or not kernel:
            decoder_hidden = self._decoder_hidden(fold, decoder_static, decoder_dynamic)
            return self._forward_bits(proj, bits, fold.dynamic_encoder, decoder_hidden, last_hh, rec, torch_only=static)
        if hm is not None:
            h_new, q = _decoder_step_heightmap(decoder_static if Ks else None, decoder_dynamic, None if last_hh is None else last_hh[0],
                                               hm, fold.P, fold.c, fold.w_hh, fold.b_hh, fold.Wq, rec)
        else:
            h_new, q = _decoder_step(decoder_static if Ks else None, decoder_dynamic if Kd else None,
                                     None if last_hh is None else last_hh[0], fold.P, fold.c, fold.w_hh, fold.b_hh, fold.Wq, rec)
        if pick is not None and static and not (torch.is_grad_enabled() and any(
                v.requires_grad for v in (proj.G, proj.g, fold.M, fold.k, q, fold.va, fold.vp))):
            current_mask, source, want_logits = pick
            return pointer_pick_static(proj.xs, bits, proj.G, proj.g, fold.M, fold.k, q, fold.va, fold.vp, current_mask, source,
                                       rows=fold.rows, want_logits=want_logits) + (h_new.unsqueeze(0),)
        if static:
            logits = pointer_scores_static(proj.xs, bits, proj.G, proj.g, fold.M, fold.k, q, fold.va, fold.vp, rows=fold.rows)
        else:
            logits = pointer_scores(proj, bits, fold.M, fold.k, q, fold.va, fold.vp, rows=fold.rows)
        return logits, h_new.unsqueeze(0)


class _Conv1x1(nn.Module):
    """The reference's Encoder (model.py:9-18): its only layer is ``conv``, a Conv1d(input_size, hidden_size, 1)"""

    def __init__(self, input_size, hidden_size):
        super(_Conv1x1, self).__init__()
        self.conv = nn.Conv1d(input_size, int(hidden_size), kernel_size=1)

    def forward(self, input):
        return self.conv(input)


class _CriticAttention(nn.Module):
    """The reference's criticAttention (trainer.py:18-42) as a parameter holder: ``v`` (1, 1, H) and ``W`` (1, H, 3 H),
    columns [static | dynamic | decoder]; StateCritic.forward does its arithmetic."""

    def __init__(self, hidden_size):
        super(_CriticAttention, self).__init__()
        self.v = nn.Parameter(torch.zeros((1, 1, hidden_size), requires_grad=True))
        self.W = nn.Parameter(torch.zeros((1, hidden_size, 3 * hidden_size), requires_grad=True))


class CriticFold(object):
    """What ``StateCritic.fold`` returns: G (3 H, S), g (3 H,), M (H, rows), v, w2 (H,), b2 (1,) -- ``rollout.critic_value``'s
    parameters -- and Wq (H, H), the attention's columns for the decoder (q0 = rnn_out . Wq^T)."""
    __slots__ = ("G", "g", "M", "v", "w2", "b2", "Wq")


class StateCritic(nn.Module):
    """The reference trainer's critic ``realCritic`` (trainer.py:44-94; its criticAttention, trainer.py:18-42) with a second
    input form.  The constructor is the reference's and so are its 16 state-dict keys -- ``static_encoder.conv.*``,
    ``dynamic_encoder.conv.*``, ``decoder.conv.*``, ``gru.*_l0``, ``attention.v``, ``attention.W``, ``fc.0.*``, ``fc.2.*`` --:
    a reference ``critic.pt`` loads with ``strict=True``.

    ``forward(static, dynamic, decoder_input=None, last_hh=None)`` -> (B, 1), as the reference returns.  A floating
    ``dynamic`` (B, rows, nR) runs the reference's arithmetic in torch, any dtype and device: the oracle path.  An int64
    ``dynamic`` is the bit shadow (``EpisodeStepper.dynamic_bits`` taken before step 0, or ``pack.dynamic_bits``): the
    encoders are folded into the attention's W and fc.0 (``fold()``) and ``rollout.critic_value`` computes the estimate in
    ONE launch from ``static`` and the shadow -- no static_hidden, no dynamic_hidden, no concatenation.
    ``decoder_input=None`` is the trainer's zero ``x0`` (trainer.py:213): the GRU step then runs for ONE row and serves the
    whole batch.  ``drop_hh`` touches only ``last_hh``, which the estimate does not depend on, so the device path is valid
    in training mode too.  The torch path takes over for ``num_layers > 1``, ``n_process_blocks`` outside 1..8, tensors
    off the GPU and shapes without a kernel (``rollout.critic_value_supported``); on a shadow it gets dynamic_hidden from
    ``rollout.encode_dynamic_bits`` on the GPU and from the unpacked bits elsewhere.

    ``fold()`` -> CriticFold, differentiable; under ``no_grad`` it can be built once and handed to ``forward(..., fold=f)``
    for many batches."""

    def __init__(self, static_size, dynamic_size, hidden_size, num_layers=1, n_process_blocks=3, dropout=0.2):
        super(StateCritic, self).__init__()
        self.static_encoder = _Conv1x1(static_size, hidden_size)
        self.dynamic_encoder = _Conv1x1(dynamic_size, hidden_size)
        self.decoder = _Conv1x1(static_size, hidden_size)
        self.gru = nn.GRU(hidden_size, hidden_size, num_layers, batch_first=True)
        self.attention = _CriticAttention(hidden_size)
        self.n_process_blocks = n_process_blocks
        self.fc = nn.Sequential(nn.Linear(hidden_size, hidden_size), nn.ReLU(), nn.Linear(hidden_size, 1))
        self.num_layers = num_layers
        self.drop_hh = nn.Dropout(p=dropout)
        self.static_size, self.dynamic_size, self.hidden_size = int(static_size), int(dynamic_size), int(hidden_size)

    def fold(self):
        H = self.hidden_size
        W = self.attention.W[0]
        Was, Wad, Waq = W[:, :H], W[:, H:2 * H], W[:, 2 * H:]
        Es, bs = self.static_encoder.conv.weight[:, :, 0], self.static_encoder.conv.bias
        Ed, bd = self.dynamic_encoder.conv.weight[:, :, 0], self.dynamic_encoder.conv.bias
        F1, f1 = self.fc[0].weight, self.fc[0].bias
        f = CriticFold()
        f.G = torch.cat((Was.matmul(Es), Waq.matmul(Es), F1.matmul(Es)), 0)
        f.g = torch.cat((Was.matmul(bs) + Wad.matmul(bd), Waq.matmul(bs), F1.matmul(bs) + f1), 0)
        f.M = Wad.matmul(Ed)
        f.v, f.w2, f.b2, f.Wq = self.attention.v[0, 0], self.fc[2].weight[0], self.fc[2].bias, Waq
        return f

    def _rnn_out(self, static, decoder_input, last_hh):
        """trainer.py:78-84: the decoder's encoder and the GRU step -> rnn_out (B, H), or (1, H) for the zero x0"""
        if decoder_input is None:
            w = self.decoder.conv.weight
            decoder_input = torch.zeros(1 if last_hh is None else static.shape[0], self.static_size, 1, dtype=w.dtype, device=w.device)
        rnn_out, last_hh = self.gru(self.decoder(decoder_input).transpose(2, 1), last_hh)
        if self.num_layers == 1:
            last_hh = self.drop_hh(last_hh)         # (with more layers the GRU has applied it); the estimate does not read it
        return rnn_out.squeeze(1)

    def _unpack(self, bits, nR):
        rows = self.dynamic_size
        w = bits.reshape(bits.shape[0], 2 if rows > 64 else 1, nR)
        r = torch.arange(rows, device=bits.device)
        return (w[:, r // 64, :] >> (r % 64).view(1, rows, 1)) & 1

    def forward(self, static, dynamic, decoder_input=None, last_hh=None, fold=None):
        from .rollout import critic_value, critic_value_supported, encode_dynamic_bits
        B, S, nR = static.shape
        H, n = self.hidden_size, self.n_process_blocks
        rnn_out = self._rnn_out(static, decoder_input, last_hh)
        shadow = dynamic.dtype is torch.int64
        if not shadow and not dynamic.is_floating_point():
            raise TypeError("StateCritic takes the int64 shadow or the floating `dynamic`, got %s" % (dynamic.dtype,))
        if shadow and self.num_layers == 1 and static.is_cuda and dynamic.is_cuda and self.attention.W.is_cuda and \
                critic_value_supported(self.dynamic_size, nR, H, S, n):
            f = self.fold() if fold is None else fold
            q0 = rnn_out.matmul(f.Wq.t())
            return critic_value(static, dynamic, f.G, f.g, f.M, q0, f.v, f.w2, f.b2, n, rows=self.dynamic_size).unsqueeze(1)
        conv = self.dynamic_encoder.conv
        if shadow:
            if dynamic.is_cuda and _lib.lib().tap_bits_words(self.dynamic_size, int(nR)) > 0:
                dynamic_hidden = encode_dynamic_bits(dynamic, conv.weight, conv.bias, rows=self.dynamic_size).to(conv.weight.dtype)
            else:
                dynamic_hidden = self.dynamic_encoder(self._unpack(dynamic, int(nR)).to(conv.weight.dtype))
        else:
            dynamic_hidden = self.dynamic_encoder(dynamic)
        static_hidden = self.static_encoder(static)
        if rnn_out.shape[0] != B:
            rnn_out = rnn_out.expand(B, -1)
        v, W = self.attention.v.expand(B, 1, H), self.attention.W.expand(B, H, -1)
        for _ in range(n):
            # criticAttention.forward (trainer.py:29-42)
            hidden = torch.cat((static_hidden, dynamic_hidden, rnn_out.unsqueeze(2).expand_as(static_hidden)), 1)
            prob = torch.softmax(torch.bmm(v, torch.tanh(torch.bmm(W, hidden))), dim=2)
            rnn_out = prob.bmm(static_hidden.permute(0, 2, 1)).squeeze(1)
        return self.fc(rnn_out)


realCritic = StateCritic


class StepFold(object):
    """What ``Pointer.fold_episode`` returns: the per-episode tensors of ``Pointer.forward_step`` (M, k, P, c, Wq, va, vp, the
    GRU's w_ih / w_hh / b_ih / b_hh) and, for the torch path, the encoders and how the decoder's two are combined;
    ``heightmap`` is the dynamic decoder when it is a ``HeightmapEncoder`` (it runs inside the step's launch), else None."""
    __slots__ = ("dynamic_encoder", "rows", "M", "k", "P", "c", "Wq", "va", "vp", "w_ih", "w_hh", "b_ih", "b_hh",
                 "static_decoder", "dynamic_decoder", "combine", "identity_dynamic", "heightmap")


class StaticFold(object):
    """What ``Pointer.fold_static`` returns and every step takes in ``proj``'s place: ``xs`` (B, S, nR) the rows of ``static``
    that the static encoder sees, detached and contiguous; ``G`` (3 Hd, S) and ``g`` (3 Hd,) the encoder folded into the two W
    (``rollout.pointer_scores_static``'s parameters); ``static_encoder`` for the torch path; ``nR`` and ``S``."""
    __slots__ = ("xs", "G", "g", "static_encoder", "nR", "S")

    def with_rows(self, xs):
        """-> a record sharing ``G``, ``g`` and ``static_encoder`` with this one, its ``xs`` re-pointed at other rows of the
        same shape: a rolling window's ``static[:, 1:, :]`` changes every step while the fold of the parameters does not.
        ``xs`` (B, S, nR) is kept as the view it is (detached, no copy) and must be one the fused launch can read in place: the
        last axis contiguous, the rows nR apart, the envs at least S nR apart (``rollout.pointer_pick_static``)."""
        from .rollout import _rows_view_stride
        if xs.dim() != 3 or tuple(int(v) for v in xs.shape[1:]) != (self.S, self.nR) or not xs.is_floating_point():
            raise ValueError("xs must be a floating (B, %d, %d) tensor, got %s %s" % (self.S, self.nR, xs.dtype, tuple(xs.shape)))
        if _rows_view_stride(xs) is None:
            raise ValueError("xs of shape %s has strides %s: its last axis must be contiguous, its rows %d apart and its envs at "
                             "least %d apart" % (tuple(xs.shape), tuple(xs.stride()), self.nR, self.S * self.nR))
        sf = StaticFold()
        sf.xs, sf.G, sf.g, sf.static_encoder, sf.nR, sf.S = xs.detach(), self.G, self.g, self.static_encoder, self.nR, self.S
        return sf


class StepDropout(object):
    """The random source of the pointer's two dropouts when they run inside the decoder step's launch
    (``Pointer.forward_step_dropout``; tapenv.h: tap_decoder_step_dropout has the definition): a counter-based generator keyed
    on (seed, episode, step, env, hidden row), so a step's masks are the same bytes wherever they are computed.  ``state`` is
    an int64[2] (seed, episode) ON ``device`` -- the launches read it there --, ``step`` a Python counter that becomes a
    launch argument.  ``env_offset``: the index of this batch's first env in the whole batch, so the shards of a
    data-parallel run draw disjoint masks from one seed (rank r of equal shards of B envs: ``env_offset = r * B``).

    ``next_episode()`` adds one to the episode as a torch op and resets ``step``: captured at the head of an episode's
    graph, it makes every replay draw new masks.  ``take_step(p_rnn, p_hh)`` -> the ``rollout.StepDropoutRecord`` of the
    next step, and advances ``step``."""

    def __init__(self, seed, device, env_offset=0):
        seed, env_offset = int(seed), int(env_offset)
        if not 0 <= seed < 1 << 63 or env_offset < 0:
            raise ValueError("seed must lie in [0, 2^63) and env_offset must not be negative, got %d and %d" % (seed, env_offset))
        self.state = torch.tensor([seed, 0], dtype=torch.int64, device=device)
        self.env_offset = env_offset
        self.step = 0
        self.pick = 0

    def next_episode(self):
        self.state[1] += 1
        self.step = 0
        self.pick = 0

    def take_pick(self):
        """-> the ``rollout.PickRecord`` of the head's next DRAW pick (``rollout.pointer_pick_draw``), and advances ``pick``: a
        counter of its own beside ``step``, so an episode may mix dropout steps and picks in any order.  The pick's Philox
        counter has the hidden row 0xFFFFFFFF, which no dropout launch has: one state feeds both without overlap."""
        from .rollout import PickRecord
        rec = PickRecord(self.state, self.pick, self.env_offset)
        self.pick += 1
        return rec

    def take_step(self, p_rnn=0.0, p_hh=0.0):
        from .rollout import StepDropoutRecord
        rec = StepDropoutRecord(self.state, self.step, float(p_rnn), float(p_hh), self.env_offset)
        self.step += 1
        return rec


class DRL(nn.Module):
    """The reference's actor (model.DRL, model.py:141-515) as ONE module that owns the episode: the constructor takes the
    reference's positional arguments, the children carry its names and shapes -- ``static_encoder``, ``dynamic_encoder`` (their
    only child ``conv``), ``decoder`` / ``dynamic_decoder`` / ``static_decoder`` + ``dynamic_decoder`` by ``decoder_input_type``
    (a ``HeightmapEncoder`` for ``block_dim == 3``), ``pointer`` (a ``Pointer``) --, so ``load_state_dict(torch.load('actor.pt'),
    strict=True)`` works on the whole module; every parameter with more than one axis is xavier-uniform, as there.
    ``update_fn`` / ``mask_fn``: ``pack.update_dynamic`` / ``pack.update_mask`` or None -- the stepper does both; another
    callable raises NotImplementedError, and so do the input types 'mul', 'mul-with' and 'use-pnet' (the two-container episode
    and the encoder RNN).  Keyword-only: ``seed`` and ``env_offset`` of the module's ``StepDropout``, ``fold`` 'static'
    (``Pointer.fold_static``: no static_hidden, no proj) or 'proj' (``Pointer.project_static``).

    ``forward(static, dynamic, decoder_input, last_hh=None, *, tour=None, stepper=None, check='nan')`` -> (tour_idx (B, n)
    int64, tour_logp (B, n) float32, None, -scores (B,)), the reference's tuple (model.py:515).  One call is one episode of
    exactly n steps -- every step retires one block, so no host read decides when to stop.  In order: ``stepper.begin``; in
    training mode ``next_episode()`` on the module's ``StepDropout`` (a torch op); the folds, once (``fold_static`` or
    ``project_static``, ``fold_decoder``, ``fold_episode``); then per step ``Pointer.forward_step`` (eval, or p = 0) or
    ``forward_step_dropout`` (training, p > 0), the head, ``stepper.step(ptr)``.  The head: ``rollout.pointer_pick_given`` on
    ``tour[:, k]`` when a ``tour`` (B, n) is passed (teacher forcing, in either mode), else greedy ``pointer_pick`` in eval
    and ``pointer_pick_draw`` from the module's ``StepDropout`` in training: torch's generator is never touched.  The first
    step's decoder input is ``decoder_input`` (a pair for the 'heightmap' types, trainer.py:116-119); ``last_hh=None`` is zeros.
    These are the launches of the hand-written recipe and no others; under ``pack.set_binary_check(
    'trust')`` and ``check`` 'nan' or False nothing is read on the host, and the whole call can be captured in one graph: the
    episode counter advances inside it, so every replay draws new masks and new picks.

    Off the GPU -- and wherever ``Pointer.forward_step`` takes its torch path -- the step is torch, and off the GPU the head is
    ``rollout.pointer_pick_torch`` with ``rollout.pick_uniforms``: the module in ``double()`` is then its own float64 model
    (a ``stepper=`` must be given there: the package's steppers live on the device).

    Kept between calls: one ``BatchedContainer`` + ``EpisodeStepper(expand_dynamic=False)`` per (shapes, device) -- ``tour_idx``
    is that stepper's buffer, valid until the next ``forward`` with these shapes: clone what must outlive it -- and one
    ``StepDropout`` per device (``step_dropout(device)``).  ``stepper=``: a ``pack.EpisodeStepper`` or anything with its
    ``begin``, ``step``, ``steps``, ``dynamic_bits``, ``current_mask``, ``decoder_static``, ``decoder_dynamic``, ``tour``,
    ``ratio`` and ``env``."""

    def __init__(self, static_size, dynamic_size, encoder_hidden_size, decoder_hidden_size, use_cuda, input_type, allow_rot,
                 container_width, container_height, block_dim, reward_type, decoder_input_type, heightmap_type, packing_strategy,
                 update_fn, mask_fn, num_layers=1, dropout=0., unit=1, *, seed=0, env_offset=0, fold='static'):
        super(DRL, self).__init__()
        from . import pack
        if dynamic_size < 1:
            raise ValueError(':param dynamic_size: must be > 0, even if the problem has no dynamic elements')
        if input_type in ('mul', 'mul-with', 'use-pnet'):
            raise NotImplementedError("input_type %r: the two-container episode ('mul', 'mul-with') and the encoder RNN "
                                      "('use-pnet') are not built into DRL" % (input_type,))
        for name, fn, own in (("update_fn", update_fn, pack.update_dynamic), ("mask_fn", mask_fn, pack.update_mask)):
            if fn is not None and fn is not own:
                raise NotImplementedError("%s: the stepper updates dynamic and the masks inside its launch; pass pack.%s or None, "
                                          "not %r" % (name, own.__name__, fn))
        if decoder_input_type not in ('shape_only', 'heightmap_only', 'shape_heightmap'):
            raise ValueError("decoder_input_type must be 'shape_only', 'heightmap_only' or 'shape_heightmap', not %r" % (decoder_input_type,))
        if fold not in ('static', 'proj'):
            raise ValueError("fold must be 'static' or 'proj', not %r" % (fold,))
        self.update_fn, self.mask_fn = update_fn, mask_fn
        self.static_encoder = _Conv1x1(static_size, encoder_hidden_size)
        self.dynamic_encoder = DynamicBitsEncoder(dynamic_size, encoder_hidden_size)
        # model.py:189-202
        heightmap_num = 1
        heightmap_width = heightmap_length = container_width * unit
        if heightmap_type == 'diff':
            if block_dim == 2:
                heightmap_width = container_width * unit - 1
            elif block_dim == 3:
                heightmap_num = 2
        heightmap_width, heightmap_length = math.ceil(heightmap_width), math.ceil(heightmap_length)

        def dynamic_decoder(hidden):
            if block_dim == 3:
                return HeightmapEncoder(heightmap_num, int(hidden), (heightmap_width, heightmap_length))
            return _Conv1x1(heightmap_width, int(hidden))
        if decoder_input_type == 'shape_only':
            self.decoder = _Conv1x1(static_size, decoder_hidden_size)
        elif decoder_input_type == 'heightmap_only':
            self.dynamic_decoder = dynamic_decoder(decoder_hidden_size)
        else:
            self.static_decoder = _Conv1x1(static_size, int(decoder_hidden_size / 2))
            self.dynamic_decoder = dynamic_decoder(decoder_hidden_size / 2)
        self.pointer = Pointer(encoder_hidden_size, decoder_hidden_size, decoder_input_type, input_type, num_layers, dropout)
        for p in self.parameters():
            if len(p.shape) > 1:
                nn.init.xavier_uniform_(p)
        self.encoder_hidden_size, self.decoder_hidden_size = encoder_hidden_size, decoder_hidden_size
        self.use_cuda, self.input_type, self.allow_rot, self.block_dim = use_cuda, input_type, allow_rot, block_dim
        self.static_size, self.dynamic_size, self.reward_type = static_size, dynamic_size, reward_type
        self.container_width, self.container_height = math.ceil(container_width * unit), container_height
        self.decoder_input_type, self.heightmap_type, self.packing_strategy = decoder_input_type, heightmap_type, packing_strategy
        self.seed, self.env_offset, self.fold = int(seed), int(env_offset), fold
        self._dropouts, self._steppers = {}, {}
        self.last_stepper = None            # the stepper of the latest forward: its check() reads the containers' error words

    def step_dropout(self, device):
        """the module's ``StepDropout`` on ``device`` (made at the first call: seed, episode 0)"""
        device = torch.device(device)
        if device not in self._dropouts:
            self._dropouts[device] = StepDropout(self.seed, device, self.env_offset)
        return self._dropouts[device]

    def _own_stepper(self, static, dynamic, n):
        from .pack import EpisodeStepper
        key = (tuple(static.shape), tuple(dynamic.shape), static.device)
        if key not in self._steppers:
            W = self.container_width
            cs = [W, self.container_height] if self.block_dim == 2 else [W, W, self.container_height]      # model.py:278-281
            env = BatchedContainer(int(static.shape[0]), cs, n, self.reward_type, self.heightmap_type,
                                   packing_strategy=self.packing_strategy, device=static.device)
            self._steppers[key] = EpisodeStepper(static, dynamic, env, self.input_type, self.allow_rot, steps=n, expand_dynamic=False)
        return self._steppers[key]

    def forward(self, static, dynamic, decoder_input, last_hh=None, *, tour=None, stepper=None, check='nan'):
        from .rollout import (_flagged_reward, pick_uniforms, pointer_pick, pointer_pick_draw, pointer_pick_given,
                              pointer_pick_torch)
        n = int(dynamic.shape[-1]) // ((2 if self.block_dim == 2 else 6) if self.allow_rot else 1)       # model.py:269-276
        B = int(static.shape[0])
        sp = stepper if stepper is not None else self._own_stepper(static, dynamic, n)
        if int(sp.steps) != n:
            raise ValueError("the stepper was built for %d steps per episode, not %d" % (sp.steps, n))
        if tour is not None:
            if tuple(tour.shape) != (B, n):
                raise ValueError("tour must be (%d, %d), got %s" % (B, n, tuple(tour.shape)))
            tour = tour.to(torch.int64).t().contiguous()            # step-major: a step's picks are a contiguous row
        sp.begin(static, dynamic)
        # (the children straight from the registry and the plain attribute through __dict__: nn.Module's attribute protocol costs
        #  about a microsecond per access, and an eval episode at c2 is short enough for ten of them to show)
        self.__dict__['last_stepper'] = sp
        mods = self._modules
        drop = None
        if self.training:
            drop = self.step_dropout(static.device)
            drop.next_episode()
        pointer, static_encoder = mods['pointer'], mods['static_encoder']
        xs = static if self.input_type == 'rot-old' else static[:, 1:, :]                                 # model.py:318-337
        proj = pointer.fold_static(static_encoder, xs) if self.fold == 'static' else pointer.project_static(static_encoder(xs))
        P, c = pointer.fold_decoder(mods.get('decoder', mods.get('static_decoder')), mods.get('dynamic_decoder'), combine='cat')
        fold = pointer.fold_episode(mods['dynamic_encoder'], P, c)
        if self.decoder_input_type == 'shape_heightmap':
            decoder_static, decoder_dynamic = decoder_input
        elif self.decoder_input_type == 'shape_only':
            decoder_static, decoder_dynamic = decoder_input, None
        else:
            decoder_static, decoder_dynamic = None, decoder_input[1] if isinstance(decoder_input, (tuple, list)) else decoder_input
        dropping = self.training and (pointer.drop_rnn.p > 0 or pointer.drop_hh.p > 0)
        logps = []
        for k in range(n):
            bits, cur = sp.dynamic_bits, sp.current_mask
            if dropping:
                logits, last_hh = pointer.forward_step_dropout(proj, bits, fold, decoder_static, decoder_dynamic, last_hh, drop)
            else:
                logits, last_hh = pointer.forward_step(proj, bits, fold, decoder_static, decoder_dynamic, last_hh)
            if not logits.is_cuda:
                u = None if drop is None or tour is not None else pick_uniforms(*drop.take_pick()[:2], B, drop.env_offset)
                ptr, logp = pointer_pick_torch(logits, cur, u, None if tour is None else tour[k])
            elif tour is not None:
                ptr = tour[k]
                logp = pointer_pick_given(logits, cur, ptr)
            elif drop is not None:
                ptr, logp = pointer_pick_draw(logits, cur, drop)
            else:
                ptr, logp = pointer_pick(logits, cur)
            logps.append(logp)
            sp.step(ptr)
            if self.decoder_input_type != 'heightmap_only':
                decoder_static = sp.decoder_static
            if self.decoder_input_type != 'shape_only':
                decoder_dynamic = sp.decoder_dynamic
        return sp.tour, torch.stack(logps, dim=1), None, _flagged_reward(-sp.ratio, check, sp.env)


class RollingDRL(DRL):
    """The reference's rolling actor (rolling.DRL, rolling.py:201-460, driven by rolling.validate's loop, rolling.py:589-637) as
    ONE module that owns the rolling episode: a trained ``child``-block actor packs N >= child blocks by sliding a window over
    the precedence graph.  The constructor is the reference's, argument for argument -- ``model.DRL``'s with ``containers``
    between ``packing_strategy`` and ``update_fn`` --; ``containers`` may be None or anything else and is ignored: the module
    keeps its own ``BatchedContainer`` (``last_env`` after a call).  The children are ``DRL``'s, so a trainer's ``actor.pt``
    loads with ``strict=True``; in 2D these are rolling.DRL's own names and shapes.  In 3D they are model.DRL's (a
    ``HeightmapEncoder`` from this module): the reference's ``rolling.HeightmapEncoder`` cannot be constructed there -- it
    divides a tuple by 4.  The input types ``DRL`` refuses are refused.  Keyword-only: ``seed`` and ``env_offset`` of the
    module's ``StepDropout``, and ``fused_pick``: a step's scores and pick in one launch (``Pointer.forward_step_pick``).

    ``forward(windows, decoder_input=None, last_hh=None, *, tour=None, steppers=None, check='nan', record=False)`` -> (tour_idx
    (B, N) int64 of window-local picks, tour_logp (B, N) float32, nodes (B, N) int32 global block ids in packing order, reward
    (B,)).  ``windows``: a fresh ``rolling.RollingWindows`` (``RollingDataset(...).windows``).  The whole call runs under
    ``torch.no_grad()``: rolling is inference.  One call is rolling.validate's inner loop for the whole batch: N - child
    one-step windows on a ``RollingStepper``, the hand-over to the ``EpisodeStepper`` of the last graph, ``child`` steps there
    (``rolling._run_rolling_steppers`` with ``expand_dynamic=False``); ``last_hh`` and the decoder inputs go from window to
    window; ``fold_static``'s G and g, ``fold_decoder`` and ``fold_episode`` are computed once; every step takes
    ``StaticFold.with_rows(static[:, 1:, :])`` of the current window and its shadow.  ``decoder_input=None``: the zeros the
    stepper starts from (the reference's x0).  The head: greedy in ``eval()``; in ``train()`` DRAW from the module's
    ``StepDropout`` (``next_episode()`` once per call), with dropout as ``forward_step_dropout`` applies it when p > 0; a
    ``tour`` (B, N) of window-local picks is scored through GIVEN.  With ``fused_pick`` and no ``tour`` a step is
    ``forward_step_pick`` (two launches and the stepper's), otherwise ``forward_step[_dropout]`` and the stand-alone head.
    ``record=True`` keeps each step's ``logits`` and ``last_hh`` in ``last_record``.

    Kept between calls: one container and one stepper pair per (B, N, D, child, device) -- ``steppers=`` takes the place of
    that pair, as in ``run_rolling_episode``; off the GPU it must be given -- and one ``StepDropout`` per device.  ``tour_idx``
    and ``nodes`` are the pair's buffers.  Windows without a one-word shadow (3 * child > 64, or child * R not a multiple of 4)
    raise ValueError.  In ``double()`` the module is its own float64 model, as ``DRL`` is."""

    def __init__(self, static_size, dynamic_size, encoder_hidden_size, decoder_hidden_size, use_cuda, input_type, allow_rot,
                 container_width, container_height, block_dim, reward_type, decoder_input_type, heightmap_type, packing_strategy,
                 containers, update_fn, mask_fn, num_layers=1, dropout=0., unit=1, *, seed=0, env_offset=0, fused_pick=True):
        super(RollingDRL, self).__init__(static_size, dynamic_size, encoder_hidden_size, decoder_hidden_size, use_cuda, input_type,
                                         allow_rot, container_width, container_height, block_dim, reward_type, decoder_input_type,
                                         heightmap_type, packing_strategy, update_fn, mask_fn, num_layers, dropout, unit, seed=seed,
                                         env_offset=env_offset, fold='static')
        self.fused_pick = bool(fused_pick)
        self._pairs = {}
        self.last_env = None                # the containers of the latest forward (rolling.validate reads its metrics there)
        self.last_record = None

    def _own_pair(self, rw):
        from .pack import EpisodeStepper
        from .rolling import RollingStepper
        key = (rw.B, rw.N, rw.D, rw.child, rw.device)
        if key not in self._pairs:
            W = self.container_width
            cs = [W, self.container_height] if rw.D == 2 else [W, W, self.container_height]
            env = BatchedContainer(rw.B, cs, rw.N, self.reward_type, self.heightmap_type, packing_strategy=self.packing_strategy,
                                   device=rw.device)
            roll = RollingStepper(rw, env, expand_dynamic=False)
            last = EpisodeStepper(roll._static[0], (rw.B, 3 * rw.child, rw.child * rw.R), env, steps=rw.child, tour=roll.tour,
                                  tour_col0=rw.N - rw.child, expand_dynamic=False)
            self._pairs[key] = (roll, last)
        return self._pairs[key]

    def forward(self, windows, decoder_input=None, last_hh=None, *, tour=None, steppers=None, check='nan', record=False):
        from .rolling import _run_rolling_steppers
        from .rollout import pick_uniforms, pointer_pick, pointer_pick_draw, pointer_pick_given, pointer_pick_torch
        rw = windows
        B, N, child, R = int(rw.B), int(rw.N), int(rw.child), int(rw.R)
        if 3 * child > 64 or (child * R) % 4:
            raise ValueError("RollingDRL needs windows with a one-word bit shadow: 3 * child <= 64 and child * R a multiple of 4, "
                             "got child %d, R %d" % (child, R))
        if int(rw.D) != self.block_dim:
            raise ValueError("the windows hold %dD blocks, the actor was built for block_dim %d" % (rw.D, self.block_dim))
        dev = torch.device(rw.device)
        if steppers is None:
            if dev.type != 'cuda':
                raise ValueError("off the GPU RollingDRL needs steppers=(rolling stepper, last-graph stepper): the package's "
                                 "steppers live on the device")
            steppers = self._own_pair(rw)
        roll, last = steppers
        if tour is not None:
            if tuple(tour.shape) != (B, N):
                raise ValueError("tour must be (%d, %d), got %s" % (B, N, tuple(tour.shape)))
            tour = tour.to(device=dev, dtype=torch.int64).t().contiguous()      # step-major: a step's picks are a contiguous row
        with torch.no_grad():
            mods = self._modules
            pointer, static_encoder = mods['pointer'], mods['static_encoder']
            drop = None
            if self.training:
                drop = self.step_dropout(dev)
                drop.next_episode()
            dropping = self.training and (pointer.drop_rnn.p > 0 or pointer.drop_hh.p > 0)
            P, c = pointer.fold_decoder(mods.get('decoder', mods.get('static_decoder')), mods.get('dynamic_decoder'), combine='cat')
            fold = pointer.fold_episode(mods['dynamic_encoder'], P, c)
            fused = self.fused_pick and tour is None
            kind = self.decoder_input_type
            carry = dict(base=None, last_hh=last_hh)
            logps, rec_steps = [], ([] if record else None)

            def policy(step, static, dynamic, current_mask, mask, decoder_static, decoder_dynamic):
                bits = roll.bits if step < N - child else last.dynamic_bits
                xs = static[:, 1:, :]
                if carry['base'] is None:
                    carry['base'] = pointer.fold_static(static_encoder, xs)     # G and g, once per call
                sf = carry['base'].with_rows(xs)
                if step == 0 and decoder_input is not None:
                    if kind == 'shape_heightmap':
                        decoder_static, decoder_dynamic = decoder_input
                    elif kind == 'shape_only':
                        decoder_static = decoder_input
                    else:
                        decoder_dynamic = decoder_input[1] if isinstance(decoder_input, (tuple, list)) else decoder_input
                    decoder_static = None if decoder_static is None else decoder_static.expand(B, *decoder_static.shape[1:])
                    decoder_dynamic = None if decoder_dynamic is None else decoder_dynamic.expand(B, *decoder_dynamic.shape[1:])
                ds = None if kind == 'heightmap_only' else decoder_static
                dd = None if kind == 'shape_only' else decoder_dynamic
                sd = drop if dropping else None
                if fused:
                    out = pointer.forward_step_pick(sf, bits, fold, ds, dd, carry['last_hh'], current_mask, drop, sd, want_logits=record)
                    ptr, logp, hh = out[0], out[1], out[-1]
                    logits = out[2] if record else None
                else:
                    logits, hh = pointer._forward_step(sf, bits, fold, ds, dd, carry['last_hh'], sd)
                    if not logits.is_cuda:
                        u = None if drop is None or tour is not None else pick_uniforms(*drop.take_pick()[:2], B, drop.env_offset)
                        ptr, logp = pointer_pick_torch(logits, current_mask, u, None if tour is None else tour[step])
                    elif tour is not None:
                        ptr = tour[step]
                        logp = pointer_pick_given(logits, current_mask, ptr)
                    elif drop is not None:
                        ptr, logp = pointer_pick_draw(logits, current_mask, drop)
                    else:
                        ptr, logp = pointer_pick(logits, current_mask)
                carry['last_hh'] = hh
                logps.append(logp)
                if record:
                    rec_steps.append(dict(logits=logits.clone(), last_hh=hh.clone()))
                return ptr

            out = _run_rolling_steppers(rw, policy, self.container_width, self.container_height, self.reward_type,
                                        self.heightmap_type, self.packing_strategy, False, steppers, check, expand_dynamic=False)
            self.__dict__['last_stepper'], self.__dict__['last_env'] = last, out['env']
            self.__dict__['last_record'] = rec_steps
            return out['tour_idx'], torch.stack(logps, dim=1), out['nodes'], out['reward']


class _EngineRow(object):
    """net.engines[b] after a PackRNN forward: the reference's per-instance PackEngine, read-only (get_heightap)"""

    def __init__(self, rows, b):
        self._rows, self._b = rows, b

    def get_heightap(self, heightmap_type):
        """PackEngine.get_heightap (LG_RL.py:498-515): a float64 array of W (W - 1 for 'diff') entries"""
        return self._rows.host(heightmap_type)[self._b].copy()


class _EngineRows(object):
    """The list the reference keeps in PackRNN.engines (LG_RL.py:610-614), served from the batched engine: the first
    get_heightap of a forward reads every instance's map in one transfer, the others index it."""

    def __init__(self, engine):
        self._engine, self._host = engine, {}

    def host(self, heightmap_type):
        if heightmap_type not in self._host:
            t = self._engine.get_heightaps(heightmap_type)
            self._host[heightmap_type] = t.detach().cpu().numpy().astype(np.float64)[:, :, 0]
        return self._host[heightmap_type]

    def __len__(self):
        return self._engine.batch_size

    def __getitem__(self, b):
        if not -len(self) <= b < len(self):
            raise IndexError("list index out of range")
        return _EngineRow(self, b % len(self))


class PackFold(object):
    """What ``PackRNN.fold`` returns, the parameters of ``rollout.pack_rnn_forward`` / ``_torch`` (tapenv.h:
    tap_pack_rnn_forward has the algebra): the two 1x1 convolutions folded into the GRUs' input weights -- ``Pe`` (3 Hb, 2),
    ``ce``; ``Pd_e`` (3 D, Hb), ``Pd_b`` (3 D, 2; LG only, else None), ``Pd_h`` (3 D, W'), ``cd`` --, both GRUs' hidden
    weights and the fc head as they are; ``kind`` 'G' | 'LG', ``Hb``, ``Hh``, ``D``, ``W``, ``Wp`` = W', ``heightmap_type``.
    Detached and contiguous, in the net's dtype on the net's device."""
    __slots__ = ("kind", "Hb", "Hh", "D", "W", "Wp", "heightmap_type") + _lib.PACK_RNN_WEIGHTS + ("_struct",)

    def weights(self, device):
        """the launch's tap_pack_rnn_weights (built once; the record keeps the tensors it points to alive)"""
        if getattr(self, "_struct", None) is None:
            w = _lib.PackRnnWeights()
            w.kind = _lib.TAP_PACK_LG if self.kind == 'LG' else _lib.TAP_PACK_G
            w.Hb, w.Hh, w.W, w.form = self.Hb, self.Hh, self.W, _lib.PNET_FORMS[self.heightmap_type]
            for k in _lib.PACK_RNN_WEIGHTS:
                t = getattr(self, k)
                if t is not None and (t.dtype != torch.float32 or t.device != torch.device(device) or not t.is_contiguous()):
                    raise _lib.TapError(_lib.TAP_E_INVALID, "the fused pack-net forward takes contiguous float32 weights on %s, %s is %s on %s"
                                        % (device, k, t.dtype, t.device))
                if t is not None and t.data_ptr() % 16:                    # a view at an odd offset: the launch reads 16 bytes at a time
                    t = t.clone()
                    setattr(self, k, t)
                setattr(w, k, None if t is None else t.data_ptr())
            self._struct = w
        return self._struct


class PackRNN(nn.Module):
    """The global pack-net (pack_net/LG_RL.py: PackRNN, LG_RL.py:562-675): 'G' (reward type C+P+S-G-soft) or 'LG'
    (C+P+S-LG-soft), what the reference's DRL_RNN (model.py:749-852) and tools.calc_positions_LG_net run.  Stock PyTorch
    with the reference's constructor, parameter names and shapes, so its checkpoints load with strict=True; forward runs
    the same torch ops in the same order.  Its environment, the reference's per-instance PackEngine, is an injected
    batched engine: ``engine`` is a factory engine(B, W, H, T, heightmap_type, max_blocks_num, device) -> an object with
    PackEngines' surface (step, reward, positions, get_heightaps); the default is env.PackEngines, one HIP launch per
    inner step for the whole batch and no host read.

    forward(blocks (B, 2, T), blocks_num) -> positions (B, T, 2) int32 (x after the clamp, z; zero beyond blocks_num),
    hit_porb_log (B, blocks_num), -reward (B,) float32 of the last inner step.  Afterwards ``engines[b].get_heightap``
    answers like the reference's engines (one batched read per forward).

    ``fused`` (keyword only, also an attribute; default False): the whole forward in ONE launch
    (``rollout.pack_rnn_forward``; tapenv.h: tap_pack_rnn_forward) when the module is in eval(), its output needs no
    gradient (grad is disabled, or neither the blocks nor a parameter require one), the blocks are float32 on the GPU,
    the engine is an env.PackEngines and the shape has a kernel (Hb = Hh = 128, 2 <= W <= 64).  In every other case the
    torch path below runs."""

    def __init__(self, block_input_size, block_hidden_size, height_input_size, height_hidden_size, container_width,
                 container_height, heightmap_type, max_blocks_num=10, pack_net_type='LG', engine=None, *, fused=False):
        super(PackRNN, self).__init__()
        self.fused = bool(fused)
        self._fold = None
        if pack_net_type == 'LG':
            decoder_hidden_size = block_hidden_size + block_hidden_size + height_hidden_size    # local + global
        else:
            decoder_hidden_size = block_hidden_size + height_hidden_size                        # global
        self.encoder = nn.GRU(block_hidden_size, block_hidden_size, batch_first=True)
        self.decoder = nn.GRU(decoder_hidden_size, decoder_hidden_size, batch_first=True)
        if heightmap_type == 'diff':
            self.height_map_conv = nn.Conv1d(height_input_size - 1, height_hidden_size, kernel_size=1)
        else:
            self.height_map_conv = nn.Conv1d(height_input_size, height_hidden_size, kernel_size=1)
        self.block_conv = nn.Conv1d(block_input_size, block_hidden_size, kernel_size=1)
        self.fc = nn.Sequential(
            nn.Linear(decoder_hidden_size, decoder_hidden_size),
            nn.ReLU(),
            nn.Linear(decoder_hidden_size, container_width),
            nn.Softmax(dim=1)
        )
        self.container_width = container_width
        self.container_height = container_height
        self.max_blocks_num = max_blocks_num
        self.dropout = nn.Dropout(p=0.1)
        self.heightmap_type = heightmap_type
        self.engines = None
        self.pack_net_type = pack_net_type
        self.engine_factory = PackEngines if engine is None else engine
        self._engine = None
        self.captured_engines = []

    def reserve(self, batch_size, T, device):
        """the engine for ``batch_size`` instances of up to ``T`` blocks on ``device`` (built or grown when needed;
        a caller that knows the longest sequence sizes it once -- DRL_RNN's prefixes grow by one block per step, so a
        grown tape doubles, up to the descriptor's limit of _TAPE_MAX steps).  Replacing the engine drops the net's
        reference to the old one; an engine that a forward used under hipGraph capture stays referenced by the net
        (``captured_engines``), because replaying that graph writes into its state blob."""
        e, dev = self._engine, torch.device(device)
        if e is not None and e.batch_size == batch_size and e.T >= T and torch.device(e.device) == dev:
            return e
        cap = T if e is None or e.batch_size != batch_size else max(T, min(2 * e.T, _TAPE_MAX))
        self._engine = self.engine_factory(batch_size, self.container_width, self.container_height, cap,
                                           self.heightmap_type, self.max_blocks_num, dev)
        return self._engine

    def fold(self):
        """-> a ``PackFold``: block_conv folded into the encoder GRU's input weights, block_conv and height_map_conv into
        the decoder GRU's (tapenv.h: tap_pack_rnn_forward), in torch, detached; no parameter is added and the state-dict
        keys stay the reference's.  The record is kept until a parameter changes (its version, memory or dtype); one
        computed under hipGraph capture is not kept."""
        params = list(self.parameters())
        key = tuple((p.data_ptr(), p._version, p.dtype) for p in params)
        if self._fold is not None and self._fold[0] == key:
            return self._fold[1]
        with torch.no_grad():
            Hb, Hh = int(self.block_conv.out_channels), int(self.height_map_conv.out_channels)
            f = PackFold()
            f.kind, f.Hb, f.Hh, f.W, f.heightmap_type = self.pack_net_type, Hb, Hh, int(self.container_width), self.heightmap_type
            f.D, f.Wp = int(self.decoder.hidden_size), int(self.height_map_conv.in_channels)
            bw, bb = self.block_conv.weight[:, :, 0], self.block_conv.bias
            hw, hb = self.height_map_conv.weight[:, :, 0], self.height_map_conv.bias
            we, wd = self.encoder.weight_ih_l0, self.decoder.weight_ih_l0
            f.Pe, f.ce = we @ bw, self.encoder.bias_ih_l0 + we @ bb
            f.Pd_e = wd[:, :Hb]
            cd = self.decoder.bias_ih_l0 + wd[:, -Hh:] @ hb
            f.Pd_b = None
            if self.pack_net_type == 'LG':
                f.Pd_b = wd[:, Hb:2 * Hb] @ bw
                cd = cd + wd[:, Hb:2 * Hb] @ bb
            f.Pd_h, f.cd = wd[:, -Hh:] @ hw, cd
            f.enc_w_hh, f.enc_b_hh = self.encoder.weight_hh_l0, self.encoder.bias_hh_l0
            f.dec_w_hh, f.dec_b_hh = self.decoder.weight_hh_l0, self.decoder.bias_hh_l0
            f.fc0_w, f.fc0_b, f.fc2_w, f.fc2_b = self.fc[0].weight, self.fc[0].bias, self.fc[2].weight, self.fc[2].bias
            for k in _lib.PACK_RNN_WEIGHTS:
                t = getattr(f, k)
                if t is not None:
                    setattr(f, k, t.detach().contiguous())
        if not (params and params[0].is_cuda and torch.cuda.is_current_stream_capturing()):
            self._fold = (key, f)
        return f

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_fold'] = None                   # a cache holding device addresses: a copy folds again
        return state

    def _takes_launch(self, blocks, engine):
        """whether this forward is the one launch (the class docstring has the conditions)"""
        if not self.fused or self.training or not blocks.is_cuda or blocks.dtype != torch.float32:
            return False
        if torch.is_grad_enabled() and (blocks.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        from .rollout import pack_rnn_forward_supported
        return isinstance(engine, PackEngines) and self.encoder.weight_ih_l0.dtype == torch.float32 and \
            pack_rnn_forward_supported(self.block_conv.out_channels, self.height_map_conv.out_channels,
                                       self.container_width, self.pack_net_type)

    def forward(self, blocks, blocks_num):
        """blocks: batch_size x block-dim x blocks-num (LG_RL.py:603-675)"""
        batch_size = blocks.shape[0]
        blocks_num = int(blocks_num)
        engine = self.reserve(batch_size, blocks.shape[-1], blocks.device)   # step 0 clears (LG_RL.py:610-614)
        if blocks.is_cuda and torch.cuda.is_current_stream_capturing() and \
                not any(c is engine for c in self.captured_engines):
            self.captured_engines.append(engine)            # the graph's launches write its blob: keep it alive

        if self._takes_launch(blocks, engine):
            from .rollout import pack_rnn_forward
            hit_porb_log, _ = pack_rnn_forward(self.fold(), engine, blocks, blocks_num)
            positions = engine.positions[:, :blocks.shape[-1]]
            if blocks_num < positions.shape[1]:
                positions[:, blocks_num:] = 0
            self.engines = _EngineRows(engine)
            return positions, hit_porb_log, -engine.reward

        block_vec = self.block_conv(blocks)
        encode_rnn_out, encoder_last_hh = self.encoder(block_vec.transpose(2, 1), None)
        encoder_last_hh = self.dropout(encoder_last_hh)
        encoder_last_hh = encoder_last_hh.squeeze(0).unsqueeze(-1)

        width = self.container_width - (1 if self.heightmap_type == 'diff' else 0)
        height_map = torch.zeros(batch_size, width, 1, dtype=blocks.dtype, device=blocks.device)    # :627, :633-639
        hit_porb_log = []
        last_hh = None
        for block_index in range(blocks_num):
            height_vec = self.height_map_conv(height_map)
            if self.pack_net_type == 'LG':
                decoder_vec = torch.cat((encoder_last_hh, block_vec[:, :, block_index:block_index + 1], height_vec), dim=1)
            else:
                decoder_vec = torch.cat((encoder_last_hh, height_vec), dim=1)
            rnn_out, last_hh = self.decoder(decoder_vec.transpose(2, 1), last_hh)
            hit_map = self.fc(last_hh[0].squeeze(1))
            best = hit_map.max(1)                       # log(max) and the first argmax (:654, :659) in one op
            hit_porb_log.append(torch.log(best[0]).unsqueeze(1))
            height_map = engine.step(block_index, blocks.detach(), best[1], want_reward=block_index == blocks_num - 1)
            height_map = height_map.to(blocks.dtype)        # the engine's is float32: net.double() is the float64 model

        positions = engine.positions[:, :blocks.shape[-1]]
        if blocks_num < positions.shape[1]:
            positions[:, blocks_num:] = 0
        self.engines = _EngineRows(engine)
        hit_porb_log = torch.cat(hit_porb_log, dim=1)
        return positions, hit_porb_log, -engine.reward


# the reference's checkpoint paths, relative to its working directory (tools.py:3544-3553, 3488-3500)
PACK_NET_CHECKPOINTS = {'C+P+S-SL-soft': './pack_net/SL_rand_diff/checkpoints/199/SL.pt',
                        'C+P+S-RL-soft': './pack_net/RL_rand_diff/checkpoints/199/actor.pt',
                        'C+P+S-G-soft': './pack_net/G_rand_diff/checkpoints/199/actor.pt',
                        'C+P+S-G-gt-soft': './pack_net/G_rand_diff/checkpoints/199/actor.pt',
                        'C+P+S-LG-soft': './pack_net/LG_rand_diff/checkpoints/199/actor.pt',
                        'C+P+S-LG-gt-soft': './pack_net/LG_rand_diff/checkpoints/199/actor.pt'}
# the global pack-net's types (tools.calc_positions_LG_net, tools.py:3463-3504)
PACK_RNN_TYPES = {'C+P+S-G-soft': 'G', 'C+P+S-G-gt-soft': 'G', 'C+P+S-LG-soft': 'LG', 'C+P+S-LG-gt-soft': 'LG'}
# PackRNN's container height when the caller gives none: the descriptor's limit (only error bit 1 depends on it)
_PACK_RNN_H = 4000
# the longest tape a descriptor takes (env.hip: tap_desc_validate, n_max <= 4096)
_TAPE_MAX = 4096


def load_pack_net(reward_type, container_width, device='cuda', container_height=None, fused=False):
    """The network tools.calc_positions_net loads for ``reward_type``, in eval mode with the reference's checkpoint:
    DQN(W, True) for the SL / RL types, PackRNN(2, 128, W, 128, W, H, 'diff', pack_net_type='G' | 'LG') for the G / LG
    types (tools.py:3488-3500).  The LG checkpoint is not shipped: FileNotFoundError, as the reference's torch.load.
    ``device=None`` leaves the network on the host.  A host PackRNN fed host blocks then needs a host engine
    injected (``net.engine_factory``): the default engine, env.PackEngines, has no CPU path and raises TapError.
    ``fused`` sets the net's ``fused`` attribute: PackRNN's one-launch forward, and for the SL / RL nets DQN's one-launch
    ``pick`` (the loader's default stays False for both; a DQN built directly defaults to True)."""
    if reward_type not in PACK_NET_CHECKPOINTS:
        raise NotImplementedError("%s has no pack-net (tools.calc_positions_net)" % reward_type)
    W = int(container_width)
    if reward_type in PACK_RNN_TYPES:
        H = _PACK_RNN_H if container_height is None else int(container_height)
        net = PackRNN(2, 128, W, 128, W, H, 'diff', pack_net_type=PACK_RNN_TYPES[reward_type], fused=fused)
    else:
        net = DQN(W, True, fused=fused)
    path = PACK_NET_CHECKPOINTS[reward_type]
    if not os.path.exists(path):
        raise FileNotFoundError("%s: the %s pack-net checkpoint (tools.py:3488-3553 loads it relative to the working "
                                "directory); pass net= instead" % (path, reward_type))
    net.load_state_dict(torch.load(path, map_location='cpu'))
    return (net if device is None else net.to(_lib.resolve_device(device))).eval()


def calc_positions_LG_net(blocks, container_size, reward_type, net=None, device='cuda'):
    """tools.calc_positions_LG_net (tools.py:3463-3504) for one instance, G / LG types: one PackRNN forward (its engine
    wraps every max_blocks_num blocks) picks the columns, then LG_RL.calc_positions replays them into a fresh
    container without a wrap (LG_RL.py:678-744) and scores the replay.
    -> positions (n, 2), container=None, stable [n] bool, ratio = (C+P+S)/3, scores = [valid, box, empty, stable_num,
    max_h].  ``net=None`` loads the reference's checkpoint (load_pack_net)."""
    from .pack import episode_scores_rnn
    if reward_type not in PACK_RNN_TYPES:
        raise NotImplementedError("%s is not a global pack-net type (calc_positions_LG_net)" % reward_type)
    blocks = np.asarray(blocks).astype('int')
    n, D = blocks.shape
    if D != 2:
        raise NotImplementedError("calc_positions_LG_net is 2D (PackEngine's height-map is a row)")
    dev = _lib.resolve_device(device)
    if net is None:
        net = load_pack_net(reward_type, container_size[0], dev, container_size[1])
    static = torch.zeros(1, 3, n, dtype=torch.float32)
    static[0, 1:, :] = torch.as_tensor(blocks.T.astype(np.float32))
    tour = torch.arange(n, dtype=torch.int64).unsqueeze(0)
    ratio, scores, env = episode_scores_rnn(static.to(dev), tour.to(dev), list(container_size), net, allow_rot=False,
                                            with_env=True)
    return (env.positions[0].cpu().numpy().astype(int), None, [bool(v) for v in env.stable[0].tolist()],
            float(ratio[0].item()), [int(v) for v in scores[0].tolist()])


def calc_positions_net(blocks, container_size, reward_type, net=None, device='cuda'):
    """tools.calc_positions_net (tools.py:3506-3598) for one instance.  G / LG types go to calc_positions_LG_net, as in
    the reference.  SL / RL types: the pack-net picks every block's
    column from the raw height-map, the placement is tools.calc_one_position_net's (tapenv.h: TAP_AT_NET).
    -> positions (n, 2), container=None, stable [n] bool, ratio = (C+P+S)/3,
    scores = [valid, box, empty, stable_num, max_h].  ``net=None`` loads the reference's checkpoint."""
    from .pack import episode_scores_net
    if reward_type in PACK_RNN_TYPES:                                                   # tools.py:3528-3532
        return calc_positions_LG_net(blocks, container_size, reward_type, net=net, device=device)
    if reward_type not in PACK_NET_CHECKPOINTS:
        raise NotImplementedError("%s has no pack-net (tools.calc_positions_net)" % reward_type)
    blocks = np.asarray(blocks).astype('int')
    n, D = blocks.shape
    if D != 2:
        raise NotImplementedError("calc_positions_net is 2D here (the reference's calc_one_position_net unpacks two sides)")
    dev = _lib.resolve_device(device)
    if net is None:
        net = load_pack_net(reward_type, container_size[0], dev)
    static = torch.zeros(1, 3, n, dtype=torch.float32)
    static[0, 1:, :] = torch.as_tensor(blocks.T.astype(np.float32))
    tour = torch.arange(n, dtype=torch.int64).unsqueeze(0)
    res = episode_scores_net(static.to(dev), tour.to(dev), reward_type, list(container_size), net, allow_rot=False,
                             with_env=True)
    ratio, scores, env = res
    return (env.positions[0].cpu().numpy().astype(int), None, [bool(v) for v in env.stable[0].tolist()],
            float(ratio[0].item()), [int(v) for v in scores[0].tolist()])
