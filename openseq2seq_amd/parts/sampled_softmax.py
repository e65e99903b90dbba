"""Sampled softmax of the language model: tf.nn.sampled_softmax_loss as losses/sequence_loss.py:391-396 calls it,
on csrc/sampled_softmax.hip and the existing GEMMs (include/os2s.h states the arithmetic).

`CandidateSampler` owns the host-built bound table of one vocabulary and draws the step's candidate set on the side
stream: the draw depends on nothing but its seed, so it runs next to the recurrence. `forward` forms the [N, Spad]
sampled logits with one GEMM over the gathered rows and runs the row-loss kernel, which leaves dlogits in their
place; `backward` is the two compact GEMMs, the scatter of the sampled rows and the true-row kernel. Scatter and
true-row kernel stay on the current stream: the embedding backward adds into the same table gradient after them."""
import torch

from .. import capi
from . import streams
from .streams import on_side_stream


class CandidateSampler(object):
  def __init__(self, vocab_size, num_sampled, max_tries=None):
    capi._check_sampled(vocab_size, num_sampled)
    self.V, self.S, self.max_tries = int(vocab_size), int(num_sampled), max_tries
    self._bounds = {}

  def bounds(self, device):
    b = self._bounds.get(device)
    if b is None:
      b = self._bounds[device] = capi.sampled_softmax_bounds(self.V).to(device)
    return b

  def draw(self, seed, device):
    """(ids [Spad], num_tries [1], log_q [Spad]) on `device`, enqueued on the side stream; the consumer joins
    the side streams (`forward` does) before it reads them."""
    bounds = self.bounds(device)
    with on_side_stream(device, bounds) as side:
      cand = capi.sampled_softmax_sample(bounds, self.V, self.S, seed, self.max_tries)
      side.hand_over(*cand)
    return cand


class SampledState(object):
  """What the forward leaves for the backward of one step."""
  __slots__ = ("x", "table", "labels", "ids", "S", "V", "w_s", "dlogits", "dtrue", "row_loss")


def forward(x2d, table, bias, labels, cand, S, V, grad_scale, grad_scale_dev=None, want_grad=True):
  """x2d [N, D] bf16, table [>= V, D] bf16 (V: the logical vocabulary), bias [>= V] fp32, labels int32 [N],
  cand = CandidateSampler.draw(...). Returns (loss [1] = grad_scale * sum(row_loss), SampledState)."""
  ids, num_tries, log_q = cand
  streams.join_side_streams()          # the candidate set was drawn next to the recurrence
  w_s, b_s = capi.sampled_softmax_gather(ids, log_q, table, bias, S, V)
  logits = capi.gemm(x2d, w_s, bias=b_s)
  st = SampledState()
  st.row_loss, loss, st.dtrue = capi.sampled_softmax_loss(x2d, table, bias, labels, ids, num_tries, S, logits,
                                                          grad_scale, grad_scale_dev, want_grad, V)
  st.x, st.table, st.labels, st.ids, st.S, st.V, st.w_s = x2d, table, labels, ids, S, V, w_s
  st.dlogits = logits if want_grad else None
  return loss, st


def backward(st, dx2d, dx_accumulate, dtable, dbias):
  """dx2d [N, D] bf16 (+)= the gradient of x; dtable [V, D] / dbias fp32 += the gradients of table and bias."""
  dl, x = st.dlogits, st.x
  spad, D = st.w_s.shape
  capi.gemm(dl, st.w_s.t().contiguous(), out=dx2d, accumulate=dx_accumulate)
  dw_s = torch.zeros((spad, D), dtype=torch.float32, device=dl.device)
  capi.gemm_wgrad(x, dl, dw_s, accumulate=True)
  db_s = None
  if dbias is not None:
    db_s = torch.zeros(spad, dtype=torch.float32, device=dl.device)
    capi.colsum_finalize(capi.bn_stats(dl), None, db_s)
  capi.sampled_softmax_scatter(st.ids, dw_s, db_s, st.S, dtable, dbias, st.V)
  capi.sampled_softmax_true_bwd(x, st.table, st.labels, st.dtrue, dx2d, dtable, dbias, st.V)
