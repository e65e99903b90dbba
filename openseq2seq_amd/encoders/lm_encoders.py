"""LMEncoder — open_seq2seq/encoders/lm_encoders.py on the HIP kernels: the AWD-style LSTM language model
(Merity et al., 2017). Embedding lookup with dropout on the MATRIX (:264, os2s_embed_wdrop_fwd), a stack of
WeightDropLayerNormBasicLSTMCell layers under dynamic_rnn (parts/rnns/rnn_layers.py: LNLSTMLayer on
csrc/lnlstm.hip) with DropoutWrapper output dropout, and the tf.layers.Dense output layer, whose kernel is also the
(transposed) embedding matrix with weight_tied: the dropped matrix feeds the lookup, the undropped one the logits,
and both gradients land in the one parameter. Layer widths are H, ..., H, and emb_size for the last layer when
tied (:236-240). Infer (:404-434): one row per seed token, greedy decoding (argmax, re-embed) for up to
num_tokens_gen steps, ended early once every row has emitted end_token (impute_finished=False), the state carried
through h0 / c0 -> hT / cT, no dropout. use_cudnn_rnn runs the existing cuDNN-form LSTM kernels.

LMClassifierEncoder is the same network in the text-classification phase (fc_dim = the data layer's num_classes !=
vocab_size, :362-384): the Dense layer reads the LAST LAYER'S FINAL STATE (h, or [h, c] with use_cell_state), the
state at step len_b - 1 of each sample, and gives [B, C] logits. LMEncoder itself refuses fc_dim / use_cell_state;
LSTMLM builds the subclass when its data layer is a TextClassificationDataLayer.

LMSampledEncoder is the LM phase trained with num_sampled < vocab_size (:375-381, lstm-wkt103-mixed.py): in train
mode it stops before the output layer and hands the table, the bias and the last layer's output to
BasicSampledSequenceLoss (parts/sampled_softmax.py); LSTMLM builds it in place of LMEncoder for such a training."""
from __future__ import absolute_import, division, print_function

import math

import torch

from .encoder import Encoder
from .rnn_encoders import apply_scope_initializer, dropout_act
from .. import capi
from ..parts import sampled_softmax
from ..parts.dense import SeedSeq, bias_grad_from_rows
from ..parts.rnns.rnn_layers import BiRNNStack, LNLSTMLayer
from ..parts.sampled_softmax import CandidateSampler
from ..parts.streams import on_side_stream
from ..parts.tape import Act

CELL_SCOPE = "weight_drop_layer_norm_basic_lstm_cell"


def _round8(n):
  return -(-n // 8) * 8


def _token_name(tok):
  return tok if isinstance(tok, str) else getattr(tok, "__name__", str(tok))


class LMEncoder(Encoder):
  @staticmethod
  def get_required_params():
    return dict(Encoder.get_required_params(), **{
        'vocab_size': int, 'emb_size': int, 'encoder_layers': int, 'encoder_use_skip_connections': bool,
        'core_cell': None, 'core_cell_params': dict, 'end_token': int, 'batch_size': int,
        'use_cudnn_rnn': bool, 'cudnn_rnn_type': None,
    })

  @staticmethod
  def get_optional_params():
    return dict(Encoder.get_optional_params(), **{
        'encoder_dp_input_keep_prob': float, 'encoder_dp_output_keep_prob': float,
        'encoder_last_input_keep_prob': float, 'encoder_last_output_keep_prob': float,
        'encoder_emb_keep_prob': float, 'variational_recurrent': bool, 'time_major': bool,
        'use_swap_memory': bool, 'proj_size': int, 'num_groups': int, 'num_tokens_gen': int,
        'fc_use_bias': bool, 'seed_tokens': list, 'sampling_prob': float, 'schedule_learning': bool,
        'weight_tied': bool, 'awd_initializer': bool, 'recurrent_keep_prob': float,
        'input_weight_keep_prob': float, 'recurrent_weight_keep_prob': float, 'weight_variational': bool,
        'dropout_seed': int, 'num_sampled': int, 'fc_dim': int, 'use_cell_state': bool,
    })

  def __init__(self, params, model, name="rnn_encoder_awd", mode='train'):
    super(LMEncoder, self).__init__(params, model, name=name, mode=mode)
    p = self.params
    self._vocab_size, self._emb_size = p['vocab_size'], p['emb_size']
    self._weight_tied = p.get('weight_tied', False)
    for key, default in (('encoder_dp_input_keep_prob', 1.0), ('encoder_dp_output_keep_prob', 1.0),
                         ('encoder_last_input_keep_prob', 1.0), ('encoder_last_output_keep_prob', 1.0),
                         ('encoder_emb_keep_prob', 1.0), ('variational_recurrent', False), ('awd_initializer', False),
                         ('recurrent_keep_prob', 1.0), ('input_weight_keep_prob', 1.0),
                         ('recurrent_weight_keep_prob', 1.0), ('weight_variational', False), ('dropout_seed', 1822)):
      p[key] = p.get(key, default)
    self._fc_dim = p.get('fc_dim', self._vocab_size)
    self._num_sampled = p.get('num_sampled', self._fc_dim)
    self._lm_phase = self._fc_dim == self._vocab_size
    self._num_tokens_gen = p.get('num_tokens_gen', 200)
    self._batch_size = p['batch_size']
    if mode == 'infer' and self._lm_phase:
      self._batch_size = len(p['seed_tokens'])
    self._use_cell_state = p.get('use_cell_state', False)

  # ---------------------------------------------------------------- variables
  def _unsupported(self):
    """What this package does not build: each raises NotImplementedError naming the parameter."""
    p, training = self.params, self._mode == "train"
    self._unsupported_phase()
    if training and self._num_sampled < self._fc_dim:
      raise NotImplementedError("num_sampled < vocabulary (sampled softmax: LMSampledEncoder, which LSTMLM builds "
                                "for training; not with use_cudnn_rnn)")
    for key in ('input_weight_keep_prob', 'recurrent_weight_keep_prob', 'encoder_dp_input_keep_prob',
                'encoder_last_input_keep_prob'):
      if p[key] < 1.0:
        raise NotImplementedError("%s < 1" % key)
    for key in ('weight_variational', 'variational_recurrent', 'encoder_use_skip_connections'):
      if p.get(key, False):
        raise NotImplementedError(key)
    if p.get('time_major', False):
      raise NotImplementedError("time_major layouts (batch-major [B,T,...] only)")

  def _unsupported_phase(self):
    if not self._lm_phase:
      raise NotImplementedError("fc_dim != vocab_size (the text-classification phase: LMClassifierEncoder, which "
                                "LSTMLM builds over an IMDBDataLayer / SSTDataLayer)")
    if self._use_cell_state:
      raise NotImplementedError("use_cell_state (the text-classification phase: LMClassifierEncoder)")

  def _resolve_cells(self):
    """Checks the cell configuration; sets self.cudnn and self.last (the width of the last layer)."""
    p = self.params
    E = self._emb_size
    cp = p['core_cell_params']
    H = int(cp['num_units'])
    self.cudnn = bool(p.get('use_cudnn_rnn', False))
    if self.cudnn:
      if 'CudnnLSTM' not in _token_name(p.get('cudnn_rnn_type')):
        raise NotImplementedError("cudnn_rnn_type %s (CudnnLSTM is built)" % _token_name(p.get('cudnn_rnn_type')))
      self.last = E
    else:
      if 'WeightDropLayerNormBasicLSTMCell' not in _token_name(p['core_cell']):
        raise NotImplementedError("core_cell %s (WeightDropLayerNormBasicLSTMCell is built)" % _token_name(p['core_cell']))
      if not cp.get('layer_norm', True):
        raise NotImplementedError("core_cell_params layer_norm=False")
      self.last = E if self._weight_tied else H
    if self._weight_tied and self.last != E:
      raise ValueError("weight_tied needs a last layer of emb_size units")

  def _l2_scale(self):
    p = self.params
    if p.get('regularizer', None) is not None:
      return float((p.get('regularizer_params', {}) or {}).get('scale', 0.0))
    return 0.0

  def _add_embedding(self, store, scope):
    V, E = self._vocab_size, self._emb_size

    def init_e(shape):
      lim = math.sqrt(6.0 / (V + E))
      return (torch.rand(shape) * 2 - 1) * lim
    return store.add(scope + "/EncoderEmbeddingMatrix", (V, E), init_e, kind="dense")

  def _add_cells(self, store, scope, first):
    """The recurrent layers, then the initializers of everything created since `first`."""
    p = self.params
    E, last = self._emb_size, self.last
    cp = p['core_cell_params']
    H = int(cp['num_units'])
    nl = int(p['encoder_layers'])
    self.layers, self.stack = [], None
    if self.cudnn:
      self.stack = BiRNNStack(store, scope + "/cudnn_rnn", "lstm_cudnn", E, E, nl, bidirectional=False)
    else:
      cin = E
      for k in range(nl):
        width = last if k == nl - 1 else H
        self.layers.append(LNLSTMLayer(store, "%s/cells/cell_%d/%s" % (scope, k, CELL_SCOPE), cin, width,
                                       forget_bias=cp.get('forget_bias', 1.0), norm_gain=cp.get('norm_gain', 1.0),
                                       norm_shift=cp.get('norm_shift', 0.0)))
        cin = width
    apply_scope_initializer(store, first, p)
    if p['awd_initializer'] and not self.cudnn:
      # parts/rnns/utils.py:52-54: uniform(+-1 / sqrt(num_units)) for the cell kernels
      for layer in self.layers:
        val = 1.0 / math.sqrt(layer.H)
        for w in (layer.wx, layer.wh):
          store._inits[w.index] = (lambda shape, val=val: (torch.rand(shape) * 2 - 1) * val)

  def build(self, store):
    self._unsupported()
    p = self.params
    first = len(store.params)
    scope = "ForwardPass/" + self._name
    V = self._vocab_size
    self.Vpad = _round8(V)
    self._resolve_cells()
    last = self.last
    # the reference wires the regularizer to the Dense kernel only (:228-234)
    l2 = self._l2_scale()

    def init(shape):   # tf.layers.Dense default: glorot_uniform; vocabulary padding rows stay zero
      lim = math.sqrt(6.0 / (last + V))
      w = (torch.rand(shape) * 2 - 1) * lim
      w[:, V:, :] = 0.0
      return w

    # variables in the reference's creation order: dense/kernel, dense/bias, [EncoderEmbeddingMatrix], the cells.
    # With weight_tied the kernel's gradient is complete only after the embedding backward, the last closure to run.
    self.proj = store.add(scope + "/dense/kernel", (1, self.Vpad, last), init, kind="conv", l2=l2, logical_out=V)
    self.bias = store.add(scope + "/dense/bias", (self.Vpad,), torch.zeros(self.Vpad), kind="vector",
                          logical_out=V) if p.get('fc_use_bias', True) else None
    self.emb = None if self._weight_tied else self._add_embedding(store, scope)
    self._add_cells(store, scope, first)
    self.output_dim = V
    return self

  # ---------------------------------------------------------------- pieces
  def _table16(self):
    return self.proj.w16.view(self.Vpad, self.last) if self.emb is None else self.emb.w16.view(self._vocab_size, -1)

  def _table_grad(self):
    return self.proj.grad.view(self.Vpad, self.last) if self.emb is None else self.emb.grad.view(self._vocab_size, -1)

  def _logits(self, feat2d):
    return capi.gemm(feat2d, self.proj.w16.view(self.Vpad, self.last),
                     bias=self.bias.master if self.bias is not None else None)

  def _embed(self, ids, lens, emb_keep, emb_seed, tape):
    """The lookup in the dropped matrix: Act [B,T,E]; its backward scatters into the table's gradient."""
    B, T = ids.shape
    E = self._emb_size
    ids_flat = ids.reshape(-1).to(torch.int32).contiguous()
    cur = Act(capi.embed_wdrop_fwd(ids_flat, self._table16(), emb_keep, emb_seed).view(B, T, E), lens)
    if tape is not None:
      enc, x0 = self, cur

      def emb_backward():
        if x0.grad is not None:
          capi.embed_wdrop_bwd(ids_flat, x0.grad.reshape(B * T, E), enc._table_grad(), emb_keep, emb_seed)
        x0.grad = None

      tape.record(emb_backward, [self.emb if self.emb is not None else self.proj])
    return cur

  # ---------------------------------------------------------------- train / eval
  def _encode(self, input_dict):
    if self._mode == "infer":
      return self._generate(input_dict)
    p = self.params
    ids, lens = input_dict['source_tensors'][0], input_dict['source_tensors'][1]
    B, T = ids.shape
    training = self._mode == "train"
    tape = input_dict.get('tape') if training else None
    seeds = input_dict.get('seeds') or SeedSeq(p['dropout_seed'])
    keep = (lambda k: p[k]) if training else (lambda k: 1.0)
    V, E, last = self._vocab_size, self._emb_size, self.last
    cur = self._embed(ids, lens, keep('encoder_emb_keep_prob'), seeds.next(), tape)
    if self.cudnn:
      cur = self.stack.forward(cur, lens, tape)
    else:
      nl = len(self.layers)
      for k, layer in enumerate(self.layers):
        y = layer.forward(cur, lens, tape, keep_prob=keep('recurrent_keep_prob'), seed=seeds.next())
        okeep = keep('encoder_last_output_keep_prob' if k == nl - 1 else 'encoder_dp_output_keep_prob')
        cur = dropout_act(y, okeep, seeds.next(), tape)
    feat = cur.data.reshape(B * T, last)
    logits2 = self._logits(feat)
    logits = Act(logits2.view(B, T, self.Vpad), lens)
    if tape is not None:
      enc, top = self, cur

      def backward():
        dl = logits.grad.reshape(B * T, enc.Vpad)
        g = top.grad_buffer()
        capi.gemm(dl, enc.proj.wt16.view(last, enc.Vpad), out=g.view(B * T, last), accumulate=top.grad_init)
        top.grad_init = True
        with on_side_stream(dl.device, dl, feat):
          capi.gemm_wgrad(feat, dl, enc.proj.grad.view(enc.Vpad, last), accumulate=True)
          if enc.bias is not None:
            bias_grad_from_rows(dl, enc.bias)
        logits.grad = None

      tape.record(backward, ([] if self._weight_tied else [self.proj]) + ([self.bias] if self.bias is not None else []))
    out = logits.data[:, :, :V]
    return {'logits': logits.data, 'logits_act': logits, 'vocab_size': V, 'outputs': [out], 'src_lengths': lens,
            'seeds': seeds}

  # ---------------------------------------------------------------- infer
  def _generate(self, input_dict):
    """GreedyEmbeddingHelper(start_tokens = seed_tokens, end_token) + BasicDecoder(zero state, output layer) +
    dynamic_decode(impute_finished=False, maximum_iterations = num_tokens_gen)."""
    p = self.params
    dev = self.proj.w16.device
    V, E = self._vocab_size, self._emb_size
    tok = torch.tensor([int(t) for t in p['seed_tokens']], dtype=torch.int32, device=dev)
    B = tok.numel()
    finished = torch.zeros(B, dtype=torch.bool, device=dev)
    lengths = torch.zeros(B, dtype=torch.int32, device=dev)
    state = [(None, None)] * len(self.layers)
    prefix = tok.view(B, 1)
    all_logits, all_ids = [], []
    for _ in range(self._num_tokens_gen):
      if self.cudnn:
        # the cuDNN-form kernels take no initial state: the growing prefix is run again each step
        n = prefix.shape[1]
        x = capi.embed_wdrop_fwd(prefix.reshape(-1).contiguous(), self._table16(), 1.0, 0).view(B, n, E)
        x = self.stack.forward(Act(x, requires_grad=False), None, None).data[:, -1].contiguous()
      else:
        x = capi.embed_wdrop_fwd(tok, self._table16(), 1.0, 0)
        for k, layer in enumerate(self.layers):
          x, h, c = layer.step(x, *state[k])
          state[k] = (h, c)
      logits = self._logits(x)
      nxt = capi.argmax_rows(logits, V)
      all_logits.append(logits[:, :V])
      all_ids.append(nxt)
      lengths += (~finished).to(torch.int32)
      finished = finished | (nxt == int(p['end_token']))
      tok = nxt
      prefix = torch.cat([prefix, nxt.view(B, 1)], dim=1)
      if bool(finished.all()):
        break
    ids = torch.stack(all_ids, dim=1)
    return {'logits': torch.stack(all_logits, dim=1), 'outputs': [ids], 'final_state': state,
            'final_sequence_lengths': lengths}

  @property
  def vocab_size(self):
    return self._vocab_size

  @property
  def emb_size(self):
    return self._emb_size


class LMClassifierEncoder(LMEncoder):
  """The text-classification phase (fc_dim != vocab_size). Variables in the reference's creation order: dense/kernel
  [D, C] (D = last, or 2 last with use_cell_state; stored [C, D]), dense/bias [C], EncoderEmbeddingMatrix [V, E]
  (always its own variable here, also with weight_tied, :255-262), the cells. DropoutWrapper drops OUTPUTS, so the
  last layer's encoder_last_output_keep_prob never reaches the classifier; the lower layers' output dropout does.
  The head is csrc/text_cls.hip: logits [B, C] fp32 from the two fp32 state pointers, and its backward hands dhT /
  dcT to os2s_lnlstm_layer_bwd_state of the top layer, which gets no gradient on y. Train, eval and infer run the
  same graph."""

  def __init__(self, params, model, name="rnn_encoder_awd", mode='train'):
    super(LMClassifierEncoder, self).__init__(params, model, name=name, mode=mode)
    if 'fc_dim' not in self.params:
      raise ValueError("LMClassifierEncoder needs fc_dim (the number of classes)")
    self._lm_phase = False
    self._batch_size = self.params['batch_size']

  def _unsupported_phase(self):
    if self.params.get('use_cudnn_rnn', False):
      raise NotImplementedError("use_cudnn_rnn in the text-classification phase (the final state of the cuDNN-form "
                                "kernels is not exposed)")
    if not 2 <= self._fc_dim <= 16:
      raise NotImplementedError("fc_dim %d (the classification head is built for 2 .. 16 classes)" % self._fc_dim)

  def build(self, store):
    self._unsupported()
    p = self.params
    first = len(store.params)
    scope = "ForwardPass/" + self._name
    self.Vpad = _round8(self._vocab_size)
    self._resolve_cells()
    C, D = self._fc_dim, (2 if self._use_cell_state else 1) * self.last

    def init(shape):   # tf.layers.Dense default: glorot_uniform
      return (torch.rand(shape) * 2 - 1) * math.sqrt(6.0 / (D + C))

    self.proj = store.add(scope + "/dense/kernel", (1, C, D), init, kind="conv", l2=self._l2_scale())
    self.bias = store.add(scope + "/dense/bias", (C,), torch.zeros(C), kind="vector") \
        if p.get('fc_use_bias', True) else None
    self.emb = self._add_embedding(store, scope)
    self._add_cells(store, scope, first)
    self.output_dim = C
    return self

  def _encode(self, input_dict):
    p = self.params
    ids, lens = input_dict['source_tensors'][0], input_dict['source_tensors'][1]
    training = self._mode == "train"
    tape = input_dict.get('tape') if training else None
    seeds = input_dict.get('seeds') or SeedSeq(p['dropout_seed'])
    keep = (lambda k: p[k]) if training else (lambda k: 1.0)
    lens = lens.to(torch.int32).contiguous()
    cur = self._embed(ids, lens, keep('encoder_emb_keep_prob'), seeds.next(), tape)
    nl = len(self.layers)
    state_grad = {}
    for k, layer in enumerate(self.layers):
      if k < nl - 1:
        y = layer.forward(cur, lens, tape, keep_prob=keep('recurrent_keep_prob'), seed=seeds.next())
        cur = dropout_act(y, keep('encoder_dp_output_keep_prob'), seeds.next(), tape)
      else:
        _, hT, cT = layer.forward(cur, lens, tape, keep_prob=keep('recurrent_keep_prob'), seed=seeds.next(),
                                  want_state=True, state_grad=state_grad)
    if not self._use_cell_state:
      cT = None
    C = self._fc_dim
    w16 = self.proj.w16.view(C, -1)
    logits = Act(capi.text_cls_fwd(hT, cT, w16, self.bias.master if self.bias is not None else None))
    if tape is not None:
      enc = self

      def backward():
        dh, dc = capi.text_cls_bwd(hT, cT, w16, logits.grad, enc.proj.grad.view(C, -1),
                                   enc.bias.grad if enc.bias is not None else None)
        state_grad.update(dhT=dh, dcT=dc)
        logits.grad = None

      tape.record(backward, [self.proj] + ([self.bias] if self.bias is not None else []))
    return {'logits': logits.data, 'logits_act': logits, 'outputs': [logits.data], 'src_lengths': lens,
            'seeds': seeds}


class LMSampledEncoder(LMEncoder):
  """The LM phase trained with num_sampled < vocab_size (:375-381): in train mode the output layer is not applied;
  the encoder hands 'weights' (enc_emb_w, the undropped [V, E] table: the transposed dense/kernel with weight_tied,
  else EncoderEmbeddingMatrix, which is then what sampled training updates), 'bias' (dense/bias), 'inputs' (the last
  layer's output) and 'num_sampled' to BasicSampledSequenceLoss. 'sampled' carries what the loss needs beside
  them: the candidate set of the step, drawn on the side stream before the recurrence is enqueued, and the hook
  that receives the loss's state for the backward closure recorded here (parts/sampled_softmax.py). Eval and infer
  are LMEncoder unchanged (the full softmax). use_cudnn_rnn keeps LMEncoder's refusal of num_sampled."""

  def _unsupported(self):
    if self._mode != "train" or self.params.get('use_cudnn_rnn', False) or not self._num_sampled < self._fc_dim:
      return super(LMSampledEncoder, self)._unsupported()
    mine, self._num_sampled = self._num_sampled, self._fc_dim
    try:
      super(LMSampledEncoder, self)._unsupported()
    finally:
      self._num_sampled = mine

  @property
  def sampled(self):
    return self._mode == "train" and self._num_sampled < self._fc_dim

  def build(self, store):
    if self.sampled:
      p, V, S = self.params, self._vocab_size, self._num_sampled
      if not p.get('fc_use_bias', True):
        raise ValueError("fc_use_bias: False with num_sampled < vocab_size (the sampled softmax reads dense/bias)")
      if not self._weight_tied and int(p['core_cell_params']['num_units']) != self._emb_size:
        raise ValueError("emb_size %d differs from the last layer's num_units %d and weight_tied is off: the sampled "
                         "softmax multiplies the last layer's output with the embedding matrix"
                         % (self._emb_size, int(p['core_cell_params']['num_units'])))
      if not (2 <= V <= capi.SAMPLED_SOFTMAX_MAX_VOCAB and 1 <= S <= V // 2):
        raise ValueError("num_sampled %d with vocab_size %d (1 <= num_sampled <= vocab_size / 2, vocab_size <= %d)"
                         % (S, V, capi.SAMPLED_SOFTMAX_MAX_VOCAB))
    super(LMSampledEncoder, self).build(store)
    if self.sampled:
      self.sampler = CandidateSampler(self._vocab_size, self._num_sampled)
    return self

  def _encode(self, input_dict):
    if not self.sampled:
      return super(LMSampledEncoder, self)._encode(input_dict)
    p = self.params
    ids, lens = input_dict['source_tensors'][0], input_dict['source_tensors'][1]
    B, T = ids.shape
    tape = input_dict.get('tape')
    seeds = input_dict.get('seeds') or SeedSeq(p['dropout_seed'])
    last = self.last
    cand = self.sampler.draw(seeds.next(), ids.device)      # depends on its seed alone: hides under the recurrence
    cur = self._embed(ids, lens, p['encoder_emb_keep_prob'], seeds.next(), tape)
    nl = len(self.layers)
    for k, layer in enumerate(self.layers):
      y = layer.forward(cur, lens, tape, keep_prob=p['recurrent_keep_prob'], seed=seeds.next())
      okeep = p['encoder_last_output_keep_prob' if k == nl - 1 else 'encoder_dp_output_keep_prob']
      cur = dropout_act(y, okeep, seeds.next(), tape)
    hook = {'candidates': cand, 'vocab_size': self._vocab_size, 'state': None}
    if tape is not None:
      enc, top = self, cur

      def backward():
        st = hook['state']
        assert st is not None, "BasicSampledSequenceLoss left no gradient for the sampled softmax"
        g = top.grad_buffer()
        sampled_softmax.backward(st, g.view(B * T, last), top.grad_init, enc._table_grad(), enc.bias.grad)
        top.grad_init = True
        hook['state'] = None

      # the table's gradient is complete only after the embedding backward; without weight_tied dense/kernel is not
      # part of the sampled graph and is final (zero) here
      tape.record(backward, [self.bias] + ([] if self._weight_tied else [self.proj]))
    return {'weights': self._table16(), 'bias': self.bias.master, 'inputs': cur.data, 'logits': cur.data,
            'outputs': [cur.data], 'num_sampled': self._num_sampled, 'sampled': hook, 'src_lengths': lens,
            'seeds': seeds}
