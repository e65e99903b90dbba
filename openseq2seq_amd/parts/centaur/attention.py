"""The attention core of Centaur's AttentionBlock on dense padded activations: softmax(scale q k^T + bias) -> dropout
-> @ v with a head dim up to 512 (csrc/attention_wide.hip), the probabilities kept as the model's alignments and a
monotonic window at inference (Attention.call, mode "loung", parts/transformer/attention_layer.py:104-220).

The q / k / v / output projections around it are Dense layers of the caller; this module owns what lies between
them.
"""
import torch

from ... import capi
from ..tape import Act, accumulate_grad

NEG_BIAS = -1e9


def padding_bias(ids):
  """get_padding_bias (parts/transformer/utils.py) without its two broadcast axes: [B, S] fp32, -1e9 where the
  source id is 0. Built from the ids, not from the lengths."""
  return (ids == 0).to(torch.float32) * NEG_BIAS


def check_shape(hidden, heads, src_len):
  """The head dims and source lengths the kernel is built for; a missing kernel is an error, never a fall-back."""
  if hidden % heads != 0:
    raise ValueError("hidden_size %d is not a multiple of %d heads" % (hidden, heads))
  d = hidden // heads
  if d not in capi.ATTENTION_WIDE_HEAD_DIMS:
    raise NotImplementedError("the dense attention kernel is built for head dims %s, not %d"
                              % (", ".join(str(x) for x in capi.ATTENTION_WIDE_HEAD_DIMS), d))
  if src_len > capi.ATTENTION_WIDE_MAX_KEYS or src_len % 8 != 0:
    raise NotImplementedError("the dense attention kernel takes a source length that is a multiple of 8 and at "
                              "most %d, not %d" % (capi.ATTENTION_WIDE_MAX_KEYS, src_len))
  return d


def wide_attention(q, k, v, key_bias, heads, tape=None, keep_prob=1.0, seed=0, positions=None, window=None,
                   back_step=0, want_argmax=False):
  """q [B, Tq, C], k / v [B, S, C] bf16 Acts (C = heads * D), key_bias [B, S] fp32. Returns (o Act [B, Tq, C],
  weights [B, heads, Tq, S] fp32 before dropout, argmax [B, heads, Tq] int32 or None). With a tape (training) the
  gradients of q, k and v are recorded; the bias and the window take none. The window applies when both
  `positions` ([B, heads, Tq] int32) and `window` are given, as in the reference."""
  B, Tq, C = q.data.shape
  S = k.data.shape[1]
  d = check_shape(C, heads, S)
  scale = float(d) ** -0.5
  if positions is None or window is None:
    positions, window, back_step = None, 0, 0
  o, p, am = capi.attention_wide_fwd(q.data, k.data, v.data, key_bias, heads, scale, keep_prob, seed, positions,
                                     window, back_step, want_argmax)
  out = Act(o, q.lens, requires_grad=tape is not None)
  if tape is not None:
    def backward():
      if out.grad is None:
        return
      dq, dk, dv = capi.attention_wide_bwd(q.data, k.data, v.data, out.grad, p, heads, scale, keep_prob, seed)
      accumulate_grad(q, dq)
      accumulate_grad(k, dk)
      accumulate_grad(v, dv)
      out.grad = None
    tape.record(backward)
  return out, p, am
