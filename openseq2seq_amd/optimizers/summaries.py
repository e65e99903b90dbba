"""The optimizer's TensorBoard summaries (post_process_gradients, optimizers.py:289-376) on the flat buffers.

On a summary step TrainOp enqueues, on the stream the update runs on and BEFORE the update reads, rescales or zeroes
anything: the statistics pass over the fp32 masters (os2s_summary_stats), the gradient multiplier 1 / (loss_scale *
world_size) from the device-resident loss scale, the statistics pass over the gradients (two passes under global-norm
clipping: sums of squares first, a one-thread kernel turns them into the clip factor on the device, then the pass with
the histograms on the clipped values). After the update the learning rate it used joins the result block and ONE
asynchronous copy takes the block to pinned memory. The block becomes events once its HIP event has completed: at the
next summary step or at close(). No parameter or gradient tensor ever travels to the host, and on every other step
nothing is launched, copied or waited for.

What counts of a variable: its logical elements where they are a leading prefix of the tensor (the vocabulary rows
of a [1, Vpad, H] projection kernel or a [Vpad] bias padded to 8; the one-unit stop projection). Where device padding
is not a prefix (the zero columns of a first recurrent layer's narrow input, `logical_in`) the whole tensor counts:
the padding holds zeros, which land in the zero bucket and in `num`.
"""
import math

import numpy as np
import torch

from .. import capi
from ..utils import summary as S

NF = len(capi.SUMMARY_STAT_FIELDS)


def logical_count(p):
  """Leading elements of variable p that are real (see the module docstring)."""
  lo = getattr(p, "logical_out", None)
  if lo is None:
    return p.numel
  if len(p.shape) == 1:
    return min(int(lo), p.numel)
  if len(p.shape) == 3 and p.shape[0] == 1:
    return min(int(lo) * p.shape[2], p.numel)
  return p.numel


class OptimizerSummaries(object):
  def __init__(self, store, cfg, summaries, larc_params=None, automatic_loss_scaling=False):
    self.store, self.cfg = store, cfg
    self.kinds = set(summaries or ())
    self.larc_params = larc_params
    self.auto_scale = bool(automatic_loss_scaling)
    self.writer = None
    dev = store.device
    nt = len(store.params)
    self.nt = nt
    counts = [logical_count(p) for p in store.params]
    self.counts = counts
    self.max_count = max(counts)
    self.counts_dev = torch.tensor(counts, dtype=torch.int64, device=dev)
    self.select = torch.ones(nt, dtype=torch.uint8, device=dev)
    k = self.kinds
    self.want_var = bool(k & {"variables", "variable_norm", "larc_summaries"})
    self.want_grad = bool(k & {"gradients", "gradient_norm", "global_gradient_norm", "larc_summaries"})
    self.want_var_hist = "variables" in k
    self.want_grad_hist = "gradients" in k
    self.clip = float(cfg.clip_global_norm) if cfg.clip_global_norm > 0 else 0.0
    # the result block: three stat tables (variables, gradients before clipping, gradients), four floats
    # (loss scale, learning rate, the two gradient multipliers), two histogram tables
    nb = capi.summary_num_buckets()
    stat_bytes = nt * NF * 8
    self._o_scal = 3 * stat_bytes
    self._o_hist = self._o_scal + 16
    hist_bytes = nt * nb * 4
    total = self._o_hist + hist_bytes * (int(self.want_var_hist) + int(self.want_grad_hist))
    self.block = torch.zeros(total, dtype=torch.uint8, device=dev)
    self.host = torch.zeros(total, dtype=torch.uint8)
    if self.block.is_cuda:
      self.host = self.host.pin_memory()
    st = lambda i: self.block[i * stat_bytes:(i + 1) * stat_bytes].view(torch.float64).view(nt, NF)
    self.st_var, self.st_pre, self.st_grad = st(0), st(1), st(2)
    self.scal = self.block[self._o_scal:self._o_scal + 16].view(torch.float32)
    o = self._o_hist
    self.hist_var = self.hist_grad = None
    if self.want_var_hist:
      self.hist_var = self.block[o:o + hist_bytes].view(torch.uint32).view(nt, nb)
      o += hist_bytes
    if self.want_grad_hist:
      self.hist_grad = self.block[o:o + hist_bytes].view(torch.uint32).view(nt, nb)
    self.workspace = capi.summary_stats_workspace(store.chunk_tensor.numel(), dev)
    self._pending = None          # (step, HIP event) of the block in flight

  # ---- device side (the update's stream is current) -----------------------------------------------------------
  def before_update(self, loss_scale_view):
    s = self.store
    kw = dict(workspace=self.workspace, max_count=self.max_count)
    if self.want_var:
      capi.summary_stats(s._master, s.chunk_tensor, s.tensor_chunk_begin, self.counts_dev, self.select, self.st_var,
                         self.hist_var, **kw)
    mult = self.scal[2:4]
    if self.want_grad:
      capi.summary_grad_mult(loss_scale_view, self.cfg.world_size, 0.0, None, self.select, mult)
      if self.clip > 0.0:
        capi.summary_stats(s._grads, s.chunk_tensor, s.tensor_chunk_begin, self.counts_dev, self.select, self.st_pre,
                           None, dev_mult=mult[0:1], **kw)
        capi.summary_grad_mult(loss_scale_view, self.cfg.world_size, self.clip, self.st_pre, self.select, mult)
      capi.summary_stats(s._grads, s.chunk_tensor, s.tensor_chunk_begin, self.counts_dev, self.select, self.st_grad,
                         self.hist_grad, dev_mult=mult[1:2], **kw)
    self.scal[0:1].copy_(loss_scale_view)

  def after_update(self, step, lr_view):
    self.scal[1:2].copy_(lr_view)
    self.host.copy_(self.block, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    self._pending = (int(step), ev)

  # ---- host side ------------------------------------------------------------------------------------------------
  def flush(self):
    """The block in flight, if any, as events (waits for its HIP event: long complete at the next summary step)."""
    if self._pending is None:
      return
    step, ev = self._pending
    self._pending = None
    ev.synchronize()
    if self.writer is None:
      return
    scalars, hists = self.events_from_block(self.host.numpy())
    self.writer.add_scalars(step, scalars)
    self.writer.add_histograms(step, hists)

  def events_from_block(self, raw):
    nt, nb, k = self.nt, capi.summary_num_buckets(), self.kinds
    stat_bytes = nt * NF * 8
    st = lambda i: raw[i * stat_bytes:(i + 1) * stat_bytes].view(np.float64).reshape(nt, NF)
    st_var, st_pre, st_grad = st(0), st(1), st(2)
    loss_scale, lr = [float(x) for x in raw[self._o_scal:self._o_scal + 8].view(np.float32)]
    o = self._o_hist
    hist_var = hist_grad = None
    if self.want_var_hist:
      hist_var = raw[o:o + nt * nb * 4].view(np.uint32).reshape(nt, nb)
      o += nt * nb * 4
    if self.want_grad_hist:
      hist_grad = raw[o:o + nt * nb * 4].view(np.uint32).reshape(nt, nb)
    scalars, hists = {}, {}
    if "learning_rate" in k:
      scalars[S.tag("learning_rate")] = lr
    if "loss_scale" in k and self.auto_scale:
      scalars[S.tag("loss_scale")] = loss_scale

    def norm(row):          # tf.norm: sqrt(sum of squares); NaN for a tensor that holds a non-finite value
      return float("nan") if row[5] > 0 else math.sqrt(row[4])

    def global_norm(table):
      return float("nan") if table[:, 5].sum() > 0 else math.sqrt(math.fsum(table[:, 4]))

    if "global_gradient_norm" in k:
      scalars[S.tag("global_gradient_norm")] = global_norm(st_pre if self.clip > 0.0 else st_grad)
      if self.clip > 0.0:
        scalars[S.tag("global_clipped_gradient_norm")] = global_norm(st_grad)
    for i, p in enumerate(self.store.params):
      if "gradients" in k:
        hists[S.tag("gradients", p.name)] = masked_histogram(st_grad[i], hist_grad[i])
      if "gradient_norm" in k:
        scalars[S.tag("gradient_norm", p.name)] = norm(st_grad[i])
      if "variables" in k:
        hists[S.tag("variables", p.name)] = (dict(zip(S.STAT_FIELDS, st_var[i])), hist_var[i])
      if "variable_norm" in k:
        scalars[S.tag("variable_norm", p.name)] = norm(st_var[i])
    if "larc_summaries" in k and self.larc_params is not None:
      for i, p in enumerate(self.store.params):
        for kind, v in S.larc_scalars(self.larc_params, lr, norm(st_var[i]), norm(st_grad[i])).items():
          scalars[S.tag(kind, p.name)] = v
    return scalars, hists


def masked_histogram(row, counts):
  """mask_nans (optimizers.py:318) applied after the fact: the pass left the non-finite gradients out and counted
  them; the reference's histogram sees each of them as 0.0."""
  stats = dict(zip(S.STAT_FIELDS, [float(x) for x in row]))
  nf = int(stats["nonfinite"])
  if nf:
    counts = np.array(counts, dtype=np.uint64)
    counts[S.ZERO_BUCKET] += nf
    stats["num"] += nf
    stats["min"], stats["max"] = min(stats["min"], 0.0), max(stats["max"], 0.0)
  return stats, counts
