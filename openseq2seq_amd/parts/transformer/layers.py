"""Building blocks of the Transformer NMT path on packed token-major tensors
(host layer over the HIP kernels; same arithmetic as
open_seq2seq/parts/transformer/{attention_layer,ffn_layer,common,embedding_layer}.py).

Every block enqueues its forward kernels and records ONE backward closure on the
Tape (see parts/tape.py). Activations are `Act` holders with 2-D bf16
data [N_tokens, hidden]. Padding never exists in this layout, so the reference's
FFN "remove_padding" (ffn_layer.py:56-70) is implicit and extends to every token-wise
op (LayerNorm, all projections), and padded keys need no -1e9 bias.
"""
import os

import torch

from ... import capi
from .. import dense, tape as _tape
from ..dense import Dense, SeedSeq      # re-exported: tests and tools reach them through this module
from ..streams import on_side_stream
from ..tape import Act


SKINNY_LOGITS = False    # [256 x 32768 x 1024]: the LDS-tiled kernel wins (60 vs 139 us)


def _accumulate_checked(x, dx):
  """tape.accumulate_grad for the norms: the input of a norm is never an activation whose gradient was finalised."""
  assert not (x.requires_grad and x.grad_masked), "a second consumer wrote to a finalised activation gradient"
  _tape.accumulate_grad(x, dx)


class LayerNorm(object):
  """LayerNormalization 'layernorm_L2' (common.py:41-68): fp32 scale/bias, eps norm_params["epsilon"] (1e-6)."""
  L1 = False

  def __init__(self, store, name, hidden, eps=1e-6):
    self.scale = store.add(name + "/layer_norm_scale", (hidden,), torch.ones(hidden), kind="vector")
    self.bias = store.add(name + "/layer_norm_bias", (hidden,), torch.zeros(hidden), kind="vector")
    self.eps = eps

  def forward(self, x, tape):
    training = tape is not None
    fwd = capi.layernorm_l1_fwd if self.L1 else capi.layernorm_fwd
    y, mean, rsave = fwd(x.data, self.scale.master, self.bias.master, self.eps, save=training)
    out = Act(y)
    if not training:
      return out
    ln = self

    def backward():
      dy = out.grad
      assert dy is not None
      dres, x.res_grad = x.res_grad, None
      if ln.L1:
        dx, partial = capi.layernorm_l1_bwd(dy, x.data, ln.scale.master, mean, rsave, dres)
      else:
        dx, _, partial = capi.layernorm_bwd(dy, x.data, ln.scale.master, mean, rsave, dres, ln.scale.grad,
                                            ln.bias.grad, defer_param_grads=True)
      with on_side_stream(dx.device, partial):      # scale / bias gradients: off the main chain
        capi.colsum_finalize(partial, ln.scale.grad, ln.bias.grad)
      _accumulate_checked(x, dx)
      out.grad = None

    tape.record(backward, [ln.scale, ln.bias])
    return out


class LayerNormL1(LayerNorm):
  """LayerNormalization 'layernorm_L1' (common.py:69-80): y = c / (mean|c| + eps) * scale + bias, c = x - mean(x);
  the same two variables as layernorm_L2. The reference's fp16 saturate_cast has no counterpart: activations are
  bf16 here, whose exponent range is fp32's."""
  L1 = True


class TokenBatchNorm(object):
  """Transformer_BatchNorm (common.py:11-38): tf.layers.batch_normalization over the [B, T, 1, D] view of the
  activations, here over the packed [N, D] tokens. Train mode normalises with the batch statistics of the N real
  tokens (the reference's also count the padded positions of its [B, T_max] batch — the one deliberate departure,
  see INTEGRATION.md) and moves moving_mean / moving_variance (TF fused-BN conventions, os2s_bn_finalize);
  eval / infer apply the moving statistics. center_scale False: no gamma / beta variables (gamma 1, beta 0)."""

  def __init__(self, store, name, hidden, training, momentum=0.95, eps=1e-4, center_scale=True, l2=0.0):
    self.D, self.training, self.momentum, self.eps = hidden, training, momentum, eps
    self.gamma = self.beta = None
    if center_scale:
      self.gamma = store.add(name + "/gamma", (hidden,), torch.ones(hidden), kind="vector", l2=l2)
      self.beta = store.add(name + "/beta", (hidden,), torch.zeros(hidden), kind="vector", l2=l2)
    dev = store.device
    self.moving_mean = torch.zeros(hidden, dtype=torch.float32, device=dev)
    self.moving_var = torch.ones(hidden, dtype=torch.float32, device=dev)
    store.add_state(name + "/moving_mean", self.moving_mean)      # checkpoints, the train -> eval copy
    store.add_state(name + "/moving_variance", self.moving_var)
    self.frozen = None

  def eval_affine(self):
    """[2, D]: scale / shift of the moving statistics (eval / infer)."""
    vec = torch.empty((2, self.D), dtype=torch.float32, device=self.moving_mean.device)
    capi.bn_finalize(None, 1, self.gamma.master if self.gamma is not None else None,
                     self.beta.master if self.beta is not None else None, self.eps, self.momentum, False,
                     self.moving_mean, self.moving_var, None, None, vec[0], vec[1])
    return vec

  def forward(self, x, tape):
    N, D = x.data.shape
    if not self.training:
      sc = self.frozen if self.frozen is not None else self.eval_affine()
      return Act(capi.token_bn_apply(x.data, sc[0], sc[1]))
    dev = x.data.device
    gamma = self.gamma.master if self.gamma is not None else None
    beta = self.beta.master if self.beta is not None else None
    vec = torch.empty((4, D), dtype=torch.float32, device=dev)      # scale, shift, mean, rstd
    capi.bn_finalize(capi.bn_stats(x.data), N, gamma, beta, self.eps, self.momentum, True, self.moving_mean,
                     self.moving_var, vec[2], vec[3], vec[0], vec[1])
    out = Act(capi.token_bn_apply(x.data, vec[0], vec[1]))
    if tape is None:
      return out
    bn = self

    def backward():
      dy = out.grad
      assert dy is not None
      dres, x.res_grad = x.res_grad, None
      partial = capi.token_bn_bwd_reduce(dy, x.data, vec[2], vec[3])
      c = torch.empty((2, D), dtype=torch.float32, device=dev)
      capi.bn_bwd_finalize(partial, 1, N, bn.gamma.grad if bn.gamma is not None else None,
                           bn.beta.grad if bn.beta is not None else None, True, c[0], c[1])
      dx = capi.token_bn_bwd_apply(dy, x.data, gamma, vec[2], vec[3], c[0], c[1], dres)
      _accumulate_checked(x, dx)
      out.grad = None

    tape.record(backward, [p for p in (bn.gamma, bn.beta) if p is not None])
    return out


class frozen_eval_norms(object):
  """Within the block, every eval-mode TokenBatchNorm of `norms` applies ONE scale / shift computed on entry from
  the moving statistics (which that mode does not change): a decode runs one launch per norm site and step, as
  LayerNorm does, instead of two. The vectors are dropped on exit, so weights copied in later are seen."""

  def __init__(self, norms):
    self.bns = [n for n in norms if isinstance(n, TokenBatchNorm) and not n.training]

  def __enter__(self):
    for n in self.bns:
      n.frozen = n.eval_affine()
    return self

  def __exit__(self, *exc):
    for n in self.bns:
      n.frozen = None
    return False


NORM_TYPES = ("layernorm_L2", "layernorm_L1", "batch_norm")


def regularizer_l2(params):
  """The scale of an l2_regularizer given as (regularizer, regularizer_params) the way the reference's Transformer
  reads it (encoders/transformer_encoder.py:71-75, common.py:19-24): 0 without a regularizer or with scale <= 0."""
  if params.get("regularizer", None) is None:
    return 0.0
  scale = float(params.get("regularizer_params", {"scale": 0.0}).get("scale", 0.0))
  return scale if scale > 0.0 else 0.0


def check_norm_params(norm_params):
  t = (norm_params or {}).get("type", "layernorm_L2")
  if t not in NORM_TYPES:
    raise ValueError("norm_params type %r: one of %s" % (t, ", ".join(NORM_TYPES)))


def make_norm(store, scope, hidden, norm_params, training):
  """The normalisation of PrePostProcessingWrapper / output_normalization (common.py:87-98): `scope` is the
  sublayer's (or the stack's) variable scope. Every kind has forward(x, tape)."""
  p = norm_params if norm_params is not None else {"type": "layernorm_L2"}
  check_norm_params(p)
  t = p.get("type", "layernorm_L2")
  if t == "batch_norm":
    cs = bool(p.get("center_scale", True))
    return TokenBatchNorm(store, scope + "/transformer__batch_norm/batch_normalization", hidden, training,
                          momentum=float(p.get("momentum", 0.95)), eps=float(p.get("epsilon", 1e-4)),
                          center_scale=cs, l2=regularizer_l2(p) if cs else 0.0)
  cls = LayerNormL1 if t == "layernorm_L1" else LayerNorm
  return cls(store, scope + "/layer_normalization", hidden, eps=float(p.get("epsilon", 1e-6)))


class MultiHeadAttention(object):
  """Attention / SelfAttention (attention_layer.py:23-227), 'loung' mode, no biases.
  Self-attention uses one fused [3D, D] projection for q,k,v; enc-dec attention a [D, D]
  query projection and a fused [2D, D] key/value projection. (The reference keeps q, k, v
  as three Dense kernels; fusing only changes how the same numbers are laid out.)"""

  def __init__(self, store, name, hidden, num_heads, self_attention, kv=None, l2=0.0):
    self.D, self.H, self.self_att = hidden, num_heads, self_attention
    if hidden % num_heads:
      raise ValueError("hidden size %d is not a multiple of num_heads %d" % (hidden, num_heads))
    self.dh = hidden // num_heads
    self.scale = self.dh ** -0.5
    if self.dh not in capi.ATTENTION_HEAD_DIMS:
      raise NotImplementedError("the HIP attention kernels are built for head dims %s, not %d (hidden %d / %d heads)"
                                % (", ".join(str(d) for d in capi.ATTENTION_HEAD_DIMS), self.dh, hidden, num_heads))
    if self_attention:
      self.qkv = Dense(store, name + "/qkv", hidden, 3 * hidden, False, l2=l2)
    else:
      self.q = Dense(store, name + "/q", hidden, hidden, False, l2=l2)
      # (the decoder creates the key / value projections of all its layers next to each other — FusedCrossKV)
      self.kv = kv if kv is not None else Dense(store, name + "/kv", hidden, 2 * hidden, False, l2=l2)
    self.out = Dense(store, name + "/output_transform", hidden, hidden, False, l2=l2)

  def forward(self, x, y, cu_q, cu_k, max_len, causal, tape, seeds, att_keep, post_keep, residual, kv_pre=None):
    """x: queries source (Act [Nq,D]); y: keys/values source (Act [Nk,D]) — y is x for
    self-attention. Returns residual + dropout(W_o attention). kv_pre = (Act [Nk, n * 2D], l): the key / value
    projections of n layers computed by ONE GEMM (FusedCrossKV), this layer's are columns [l * 2D, (l + 1) * 2D)."""
    D, H = self.D, self.H
    kv_all = None
    if self.self_att:
      qkv = self.qkv.forward(x, tape)
      qv, kv_, vv = qkv.data[:, :D], qkv.data[:, D:2 * D], qkv.data[:, 2 * D:]
    elif kv_pre is not None:
      q = self.q.forward(x, tape)
      kv_all, lidx = kv_pre
      kd = kv_all.data[:, lidx * 2 * D:(lidx + 1) * 2 * D]
      qv, kv_, vv = q.data, kd[:, :D], kd[:, D:]
    else:
      q = self.q.forward(x, tape)
      kv = self.kv.forward(y, tape)
      qv, kv_, vv = q.data, kv.data[:, :D], kv.data[:, D:]
    seed = seeds.next()
    o, lse = capi.attention_fwd(qv, kv_, vv, cu_q, cu_k, H, max_len, causal, self.scale,
                                att_keep, seed, dh=self.dh)
    oa = Act(o)
    if tape is not None:
      att = self

      def backward():
        d_o = oa.grad
        assert d_o is not None
        if att.self_att:
          g = torch.empty_like(qkv.data)
          capi.attention_bwd(qv, kv_, vv, d_o, lse, g[:, :D], g[:, D:2 * D], g[:, 2 * D:], cu_q,
                             cu_k, H, max_len, causal, att.scale, att_keep, seed, dh=att.dh)
          qkv.grad = g
        elif kv_all is not None:
          # this layer's columns of the fused gradient; FusedCrossKV's closure runs after every layer's
          gq = torch.empty_like(q.data)
          gkv = kv_all.grad_buffer()[:, lidx * 2 * D:(lidx + 1) * 2 * D]
          capi.attention_bwd(qv, kv_, vv, d_o, lse, gq, gkv[:, :D], gkv[:, D:], cu_q, cu_k, H,
                             max_len, causal, att.scale, att_keep, seed, dh=att.dh)
          q.grad = gq
        else:
          gq = torch.empty_like(q.data)
          gkv = torch.empty_like(kv.data)
          capi.attention_bwd(qv, kv_, vv, d_o, lse, gq, gkv[:, :D], gkv[:, D:], cu_q, cu_k, H,
                             max_len, causal, att.scale, att_keep, seed, dh=att.dh)
          q.grad, kv.grad = gq, gkv
        oa.grad = None

      tape.record(backward)
    return self.out.forward(oa, tape, keep=post_keep, seed=seeds.next(), residual=residual)


# A/B knob: 0 = one key / value GEMM per decoder layer (rounds 1 - 4)
FUSE_CROSS_KV = os.environ.get("OS2S_FUSE_CROSS_KV", "1") == "1"
FUSE_CROSS_KV_SIDE = os.environ.get("OS2S_FUSE_CROSS_KV_SIDE", "1") == "1"


class FusedCrossKV(object):
  """The key / value projections of the encoder output for ALL decoder layers' encoder-decoder attention
  (transformer_decoder.py:155-230: every layer projects the same encoder output with its own k, v kernels) as ONE
  GEMM with N = n_layers * 2D columns — 1584 tiles instead of six launches of 264 for Transformer-big — and ONE
  TN GEMM for the six kernel gradients. The kernels stay six variables under their reference names; they are created
  next to each other, so their bf16 copies (and their gradients) ARE the rows of one [n * 2D, D] matrix. The data
  gradient into the encoder output stays one GEMM per layer (the transposed weight copies are per kernel)."""

  def __init__(self, store, kvs):
    self.store, self.kvs = store, kvs
    self.D = kvs[0].cin

  def join(self):
    """The current stream waits for the fused projection (no-op when it ran on the current stream)."""
    if getattr(self, "_side", None) is not None:
      torch.cuda.current_stream().wait_stream(self._side)
      self._side = None

  def usable(self):
    ks = [d.kernel for d in self.kvs]
    return FUSE_CROSS_KV and len(ks) > 1 and all(b.offset == a.offset + a.numel and b.numel == a.numel
                                                 for a, b in zip(ks, ks[1:]))

  def _rows(self, flat):
    k0, n = self.kvs[0].kernel, len(self.kvs)
    return flat[k0.offset:k0.offset + n * k0.numel].view(n * 2 * self.D, self.D)

  def forward(self, enc_out, tape):
    # on the side stream: nothing of the decoder needs the result before its first encoder-decoder attention, and
    # the embedding + self-attention sublayer in front of it are 132-tile launches that leave half the chip idle
    # (the decoder calls join() there)
    self._side = None
    if FUSE_CROSS_KV_SIDE:
      with on_side_stream(enc_out.data.device, enc_out.data) as ctx:
        y = capi.gemm_nt(enc_out.data, self._rows(self.store.w16))
        ctx.hand_over(y)
        self._side = ctx.side
    else:
      y = capi.gemm_nt(enc_out.data, self._rows(self.store.w16))
    out = Act(y)
    if tape is None:
      return out
    fused, D = self, self.D

    def backward():
      g = out.grad
      assert g is not None, "no decoder layer wrote the fused key / value gradient"
      with on_side_stream(g.device, enc_out.data, g):
        capi.gemm_wgrad(enc_out.data, g, fused._rows(fused.store.grads), accumulate=True)
      if enc_out.requires_grad:
        ge = enc_out.grad_buffer()
        for l, d in enumerate(fused.kvs):
          gl = g[:, l * 2 * D:(l + 1) * 2 * D]
          if g.shape[0] < capi.BIG_TILE_MIN_ROWS:     # the small-batch kernel wants contiguous rows
            gl = gl.contiguous()
          capi.gemm(gl, d.kernel.wt16.view(d.cin, d.cout), out=ge, accumulate=enc_out.grad_init)
          enc_out.grad_init = True
      out.grad = None

    tape.record(backward, [d.kernel for d in self.kvs])
    return out


class FeedForward(object):
  """FeedFowardNetwork (ffn_layer.py:25-85): Dense(filter, relu) -> dropout -> Dense(hidden)."""

  def __init__(self, store, name, hidden, filter_size, l2=0.0):
    self.filter_layer = Dense(store, name + "/filter_layer", hidden, filter_size, True, l2=l2)
    self.output_layer = Dense(store, name + "/output_layer", filter_size, hidden, True, l2=l2)

  def forward(self, x, tape, seeds, relu_keep, post_keep, residual):
    s1, s2 = (seeds.next(), seeds.next()) if seeds is not None else (0, 0)
    h = self.filter_layer.forward(x, tape, act=1, keep=relu_keep, seed=s1)
    return self.output_layer.forward(h, tape, keep=post_keep, seed=s2, residual=residual)


class SharedEmbedding(object):
  """EmbeddingSharedWeights (embedding_layer.py:26-105): one [V, D] matrix used for the
  input embeddings of both stacks and, transposed, for the pre-softmax projection.

  pad_vocab_to_eight (the reference's pad_embeddings_2_eight) rounds V itself up: the extra rows are real, trained
  vocabulary, as in the reference. Any other V that is no multiple of 8 keeps its logical size — the variable is
  [V, D] in checkpoints (logical_out) and V is what the loss, the beam search and an argmax see (`V`) — while the
  device table has Vpad = V rounded up to 8 rows (the GEMMs' and the loss kernel's 16-byte vectors). The padding
  rows are zero and stay zero: no id selects them and their logit columns carry no probability and no gradient
  (os2s_xent_smooth V_valid), so their weight gradient is exactly zero."""

  def __init__(self, store, name, vocab_size, hidden, pad_vocab_to_eight=False):
    if pad_vocab_to_eight and vocab_size % 8:
      vocab_size += 8 - vocab_size % 8
    self.V, self.D = vocab_size, hidden
    self.Vpad = -(-vocab_size // 8) * 8
    V = vocab_size

    def init(shape):   # random_normal_initializer(0, hidden**-0.5)
      w = torch.randn(shape) * hidden ** -0.5
      w[:, V:, :] = 0.0          # vocabulary padding rows
      return w

    self.weights = store.add(name + "/embedding_and_softmax/weights", (1, self.Vpad, hidden),
                             init, kind="conv", logical_out=V if self.Vpad != V else None)

  @property
  def table(self):
    return self.weights.w16.view(self.Vpad, self.D)

  def embed(self, ids, pos, tape, keep, seed, final_use=False):
    """final_use: True for the FIRST use in forward order (= the last closure of the
    backward pass that touches the shared weights; only then are their gradients final)."""
    out = Act(capi.embed_fwd(ids, pos, self.table, self.D ** 0.5, keep, seed))
    if tape is not None:
      emb = self

      def backward():
        if out.grad is not None:
          # a parameter gradient: side stream, like every other (all three writers of the shared
          # table — the softmax weight gradient and both embedding scatters — sit on that ONE stream,
          # in order: the scatter's atomics must not interleave with the GEMM's read-modify-write)
          with on_side_stream(out.grad.device, ids, out.grad):
            capi.embed_bwd(ids, out.grad, emb.weights.grad.view(emb.Vpad, emb.D), emb.D ** 0.5, keep,
                           seed)
        out.grad = None

      tape.record(backward, [emb.weights] if final_use else ())
    return out

  def linear(self, x, tape):
    """logits = x E^T  (bf16 [N, Vpad]; columns >= V are the zero padding rows' and count nowhere)."""
    if tape is None and x.data.shape[0] <= dense.SKINNY_MAX_ROWS and SKINNY_LOGITS:
      return Act(capi.gemm_skinny(x.data, self.table))
    out = Act(capi.gemm(x.data, self.table))
    if tape is not None:
      emb = self

      def backward():
        dy = out.grad
        assert dy is not None
        g = x.grad_buffer()
        with on_side_stream(dy.device, x.data, dy):
          capi.gemm_wgrad(x.data, dy, emb.weights.grad.view(emb.Vpad, emb.D), accumulate=True)
        capi.gemm(dy, emb.weights.wt16.view(emb.D, emb.Vpad), out=g, accumulate=x.grad_init)
        x.grad_init = True
        out.grad = None

      tape.record(backward)
    return out
