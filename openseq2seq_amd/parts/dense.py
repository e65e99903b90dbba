"""The layer-level pieces every model family shares: Dense, SeedSeq and the bias gradient of a row-major activation.

`Dense` is tf.layers.Dense on packed [N, Cin] rows: `forward` enqueues the GEMM and records one backward closure on
the Tape (parts/tape.py); its weight gradient goes to the side stream (parts/streams.py), alone or collected by
`Tape.defer_wgrad`. The knobs below are read as globals of THIS module at call time: set them here, nowhere else.
`SeedSeq` numbers the dropout streams of a step; `bias_grad_from_rows` is bias.grad += column sums. The layers only
the Transformer uses are parts/transformer/layers.py.
"""
import math
import os

import torch

from .. import capi
from .streams import on_side_stream
from .tape import Act, current_tape


SKINNY_MAX_ROWS = 512
# Dense weight gradients on the side stream (as the conv families do): most Dense GEMMs of a
# Transformer-big step are 132 tiles on 256 CUs (8300 tokens x 1024 columns), the split weight
# gradient fills the other half of the chip. 22.1 -> 20.3 ms/step, sustained over 300 steps
# (OS2S_DENSE_WGRAD_STREAM=0 keeps them on the main stream)
DENSE_WGRAD_STREAM = os.environ.get("OS2S_DENSE_WGRAD_STREAM", "1") == "1"
# the ReLU + dropout backward of a Dense layer fused into the data-gradient GEMM of its consumer
# (os2s_gemm_nt_mask_ws); OS2S_FUSE_RELU_BWD=0 = the separate dropout_bwd_colsum pass of round 2
FUSE_RELU_BWD = os.environ.get("OS2S_FUSE_RELU_BWD", "1") == "1"
# Dense weight gradients with fewer than 32 output tiles of 256 x 256 (the 1024 x 1024 projections)
# are collected three at a time into one ping-pong launch (OS2S_GROUP_SMALL_WGRAD=0: one lockstep
# launch with fp32 atomics each, as in round 2)
GROUP_SMALL_WGRAD = os.environ.get("OS2S_GROUP_SMALL_WGRAD", "1") == "1"


def _small_wgrad(lin, dz):
  units = ((lin.cout + 255) // 256) * ((lin.cin + 255) // 256)
  return units < 32 and lin.cout >= 128 and lin.cin >= 128 and dz.shape[0] >= 2048 and \
      lin.cout % 8 == 0 and lin.cin % 8 == 0


# Round 6: EVERY Dense weight gradient with fewer output tiles than the chip has CUs is held back until the
# collected ones cover WGRAD_UNIT_BUDGET tiles of 256 x 256 (Transformer-big: ffn 64 + 64, q k v 48, the 1024 x 1024
# projections 16 each — 192 / 224 per encoder / decoder layer), then go out as ONE launch of the ping-pong TN-GEMM
# kernel: ~200 tiles of 130 reduction steps each and no reduction split, where the single launches were 16 - 64 tiles
# cut 4 - 16 ways (fill, 256 KB slab per piece, one reducer per tile). Transformer-big, same box, interleaved
# (ms per step): round-5 policy 18.30, budget 128: 17.56, 192: 17.27 - 17.39, 256: 17.85 — a launch that leaves a
# quarter of the CUs to the data-gradient chain on the main stream beats one that takes them all.
# OS2S_WGRAD_UNIT_BUDGET=0: the round-5 policy (1024 x 1024 projections three at a time, the rest alone).
WGRAD_UNIT_BUDGET = int(os.environ.get("OS2S_WGRAD_UNIT_BUDGET", "192"))


def _groupable_wgrad(lin, dz):
  units = ((lin.cout + 255) // 256) * ((lin.cin + 255) // 256)
  return WGRAD_UNIT_BUDGET > 0 and units < 256 and lin.cout >= 128 and lin.cin >= 128 and dz.shape[0] >= 2048 and \
      lin.cout % 8 == 0 and lin.cin % 8 == 0 and dz.stride(1) == 1


class SeedSeq(object):
  """Distinct dropout streams per op per step."""

  def __init__(self, base):
    self.base, self.n = int(base), 0

  def next(self):
    self.n += 1
    return (self.base * 1000003 + self.n) & ((1 << 62) - 1)


def bias_grad_from_rows(dy2d, bias_param):
  """bias.grad += column sums of dy (bf16 [N, C])."""
  capi.colsum_finalize(capi.bn_stats(dy2d), None, bias_param.grad)


class Dense(object):
  """tf.layers.Dense on [N, Cin] rows; kernel stored [1, Cout, Cin] (device layout,
  = the transpose of TF's [Cin, Cout])."""

  def __init__(self, store, name, cin, cout, use_bias, l2=0.0):
    self.cin, self.cout = cin, cout

    def init(shape):   # tf.layers.Dense default initializer: glorot_uniform
      lim = math.sqrt(6.0 / (cin + cout))
      return (torch.rand(shape) * 2 - 1) * lim

    # l2: the scale of the encoder's / decoder's l2_regularizer, on kernel and bias alike
    # (attention_layer.py:54-62, ffn_layer.py:36-49)
    self.kernel = store.add(name + "/kernel", (1, cout, cin), init, kind="conv", l2=l2)
    self.bias = store.add(name + "/bias", (cout,), torch.zeros(cout), kind="vector", l2=l2) \
        if use_bias else None

  @property
  def w(self):
    return self.kernel.w16.view(self.cout, self.cin)

  def forward(self, x, tape, act=0, keep=1.0, seed=0, residual=None):
    """y = residual + dropout(act(x W^T + b)); x, residual: Act; returns Act."""
    if tape is None and keep >= 1.0 and x.data.shape[0] <= SKINNY_MAX_ROWS:
      # decoding step: a few hundred rows — latency-bound kernel (csrc/gemm_skinny.hip)
      return Act(capi.gemm_skinny(x.data, self.w, bias=self.bias.master if self.bias is not None else None,
                                  relu=(act == 1), residual=residual.data if residual is not None else None))
    bias = self.bias.master if self.bias is not None else None
    res = residual.data if residual is not None else None
    if self.cin % 64 == 0 and act in (0, 1, 3) and self.cout % 8 == 0:   # what gemm_pp.hip accepts
      y = capi.gemm_nt(x.data, self.w, bias=bias, act=act, keep_prob=keep, seed=seed, residual=res)
    else:
      y = capi.gemm(x.data, self.w, bias=bias, act=act, keep_prob=keep, seed=seed, residual=res)
    out = Act(y)
    if tape is None:
      return out
    lin = self
    assert not (act in (1, 3) and residual is not None)
    if act == 1 and FUSE_RELU_BWD and y.is_contiguous():
      out.mask_scale = 1.0 / keep       # y = dropout(relu(.)): zero exactly where the gradient is

    def backward():
      dy = out.grad
      assert dy is not None, "no gradient reached " + lin.kernel.name
      bias_part = None          # partial column sums of dz when the same pass can produce them
      fuse = lin.bias is not None and dy.is_contiguous()
      if act == 1 and out.grad_masked:
        # the consumer's data-gradient GEMM applied (y > 0) / keep in its epilogue
        dz, bias_part = dy, out.bias_part
        out.bias_part = None
      elif act in (1, 3):
        # act 3 = min(relu(.), 20): no gradient where the stored output sits at the cap either
        if fuse:
          dz, bias_part = capi.dropout_bwd_colsum(dy, keep, out=y, capped=(act == 3))
        else:
          dz = capi.dropout_bwd(dy, keep, out=y, capped=(act == 3))     # (y > 0) / keep
      elif keep < 1.0:
        if fuse:
          dz, bias_part = capi.dropout_bwd_colsum(dy, keep, seed=seed)
        else:
          dz = capi.dropout_bwd(dy, keep, seed=seed)     # recomputed hash mask / keep
      else:
        dz = dy
      # dW += dz^T x (fp32) and dx (+)= dz W: plain GEMMs. The weight gradient goes to the side
      # stream by default (OS2S_DENSE_WGRAD_STREAM): with the in-tree kernels it fills the half of
      # the chip a 132-tile data-gradient GEMM leaves idle, 22.1 -> 20.3 ms/step over 20 AND over
      # 300 steps (with the round-1 vendor GEMMs the same move lost 11 % at the power limit)
      if GROUP_SMALL_WGRAD and _groupable_wgrad(lin, dz) and current_tape() is not None:
        # (OS2S_DENSE_WGRAD_STREAM=0 keeps the grouped launch on the main stream: the serial profiles)
        current_tape().defer_wgrad(lin.kernel, dict(x=x.data, dy=dz, dw=lin.kernel.grad.view(lin.cout, lin.cin)),
                                   unit_budget=WGRAD_UNIT_BUDGET, side=DENSE_WGRAD_STREAM)
      elif DENSE_WGRAD_STREAM and GROUP_SMALL_WGRAD and _small_wgrad(lin, dz) and current_tape() is not None:
        # 16 output tiles: three of these go out as ONE launch (Tape.defer_wgrad)
        current_tape().defer_wgrad(lin.kernel, dict(x=x.data, dy=dz, dw=lin.kernel.grad.view(lin.cout, lin.cin)))
      elif DENSE_WGRAD_STREAM:
        with on_side_stream(dz.device, x.data, dz):
          capi.gemm_wgrad(x.data, dz, lin.kernel.grad.view(lin.cout, lin.cin), accumulate=True)
      else:
        capi.gemm_wgrad(x.data, dz, lin.kernel.grad.view(lin.cout, lin.cin), accumulate=True)
      if bias_part is not None and lin.bias is not None:
        with on_side_stream(dz.device, bias_part):        # parameter gradient: off the main chain
          capi.colsum_finalize(bias_part, None, lin.bias.grad)
      elif lin.bias is not None:
        with on_side_stream(dz.device, dz):
          bias_grad_from_rows(dz, lin.bias)
      if x.requires_grad:
        g = x.grad_buffer()
        if x.mask_scale is not None and not x.grad_init and lin.cout % 64 == 0 and lin.cin % 8 == 0 and \
            dz.stride(1) == 1 and g.is_contiguous():
          # x = dropout(relu(.)) of the layer below, this is the only consumer: its activation
          # backward (and the bias-gradient partials) ride in this GEMM's epilogue
          _, x.bias_part = capi.gemm_nt_mask(dz, lin.kernel.wt16.view(lin.cin, lin.cout), x.data, x.mask_scale,
                                             out=g, want_colsum=True)
          x.grad_masked = True
        else:
          capi.gemm(dz, lin.kernel.wt16.view(lin.cin, lin.cout), out=g, accumulate=x.grad_init)
        x.grad_init = True
      if residual is not None:
        residual.res_grad = dy      # consumed by the pre-norm LayerNorm backward of `residual`
      out.grad = None

    tape.record(backward, [lin.kernel] + ([lin.bias] if lin.bias is not None else []))
    return out
