"""Recurrent layers on the HIP RNN kernels (csrc/rnn.hip): cuDNN-form GRU / LSTM
(tf.contrib.cudnn_rnn.CudnnGRU/CudnnLSTM, encoders/ds2_encoder.py:294-328,
encoders/tacotron2_encoder.py:254-263) and tf.nn.rnn_cell.LSTMCell under
(bidirectional_)dynamic_rnn (encoders/rnn_encoders.py:221-305, parts/rnns/utils.py:17-89).

One `RNNDirection` = one direction of one layer: the input projection of all time steps is
one MFMA GEMM per input tensor (a bidirectional lower layer is consumed as two tensors, so
no concat is materialised), the recurrence is os2s_rnn_layer_fwd/bwd, and the weight
gradients are GEMMs over the saved gate gradients (h_{t-1} enters as a time-shifted
operand of the wgrad kernel)."""
import math
import os

import torch

from ... import capi
from ..streams import on_side_stream
from ..tape import Act
from ..dense import bias_grad_from_rows

CELLS = {"gru_cudnn": capi.CELL_GRU_CUDNN, "lstm_cudnn": capi.CELL_LSTM_CUDNN,
         "lstm_tf": capi.CELL_LSTM_TF}


# rows (B x T) from which the recurrent weight gradient goes through the ping-pong TN GEMM
SHIFTED_WH_MIN_ROWS = int(os.environ.get("OS2S_RNN_WH_GEMM_ROWS", "4096"))


class RNNDirection(object):
  def __init__(self, store, name, cell, input_sizes, hidden, reverse=False, forget_bias=1.0, logical_in=None):
    """logical_in: the real width of a (single) input that the caller zero-pads to input_sizes[0]: the kernel's
    extra columns start at zero — and stay there, their inputs being zero —, the glorot limit counts the real
    fan-in and checkpoints carry the logical shape."""
    self.cell_name, self.cell = cell, CELLS[cell]
    self.H, self.G = hidden, 3 if cell == "gru_cudnn" else 4
    self.reverse, self.forget_bias = reverse, (forget_bias if cell == "lstm_tf" else 0.0)
    GH = self.G * hidden
    assert logical_in is None or (len(input_sizes) == 1 and logical_in <= input_sizes[0])
    tot_in = sum(input_sizes) if logical_in is None else logical_in

    def init_w(fan_in, live=None):
      def f(shape):   # glorot-uniform over the full [in + H, G*H] matrix (TF LSTMCell default)
        lim = math.sqrt(6.0 / (fan_in + hidden + GH))
        w = (torch.rand(shape) * 2 - 1) * lim
        if live is not None:
          w[:, :, live:] = 0
        return w
      return f

    self.wx = [store.add("%s/wx_%d" % (name, i), (1, GH, n), init_w(tot_in, logical_in), kind="conv")
               for i, n in enumerate(input_sizes)]
    if logical_in is not None:
      self.wx[0].logical_in = logical_in
    self.wh = store.add(name + "/wh", (1, GH, hidden), init_w(tot_in), kind="conv")
    self.bx = store.add(name + "/bias", (GH,), torch.zeros(GH), kind="vector")
    self.bh = store.add(name + "/bias_h", (GH,), torch.zeros(GH), kind="vector") \
        if cell != "lstm_tf" else None

  def input_projection(self, xs):
    B, T, _ = xs[0].data.shape
    GH = self.G * self.H
    gx = None
    for i, (x, w) in enumerate(zip(xs, self.wx)):
      gx = capi.gemm(x.data.reshape(B * T, -1), w.w16.view(GH, -1),
                     bias=self.bx.master if i == 0 else None, out=gx, accumulate=i > 0)
    return gx.view(B, T, GH)

  def params(self):
    return [self.wh, self.bx] + self.wx + ([self.bh] if self.bh is not None else [])

  def weight_backward(self, xs, lens, y, dgx, dgr, h_seq=None):
    """dX, dWx, dWh and the bias gradients from the saved gate gradients. h_seq: under zoneout the state
    sequence the recurrent product read (the zoned h'), which then stands in for the outputs y in dWh."""
    if h_seq is not None:
      y = h_seq
    B, T, _ = xs[0].data.shape
    H, GH = self.H, self.G * self.H
    d2 = dgx.view(B * T, GH)
    # the data gradients first, on the main stream (the layer below waits for them) ...
    for x, w in zip(xs, self.wx):
      if x.requires_grad:
        g = x.grad_buffer()
        capi.gemm(d2, w.wt16.view(-1, GH), out=g.view(B * T, -1), accumulate=x.grad_init)
        x.grad_init = True
    # ... the parameter gradients on the side stream: nothing in the rest of backward reads them, and
    # during the next layer's recurrence (ONE persistent launch on two XCDs for a DeepSpeech2 GRU layer)
    # six XCDs have nothing else to do
    with on_side_stream(dgx.device, dgx, dgr, y, *[x.data for x in xs]):
      for x, w in zip(xs, self.wx):
        capi.gemm_wgrad(x.data.reshape(B * T, -1), d2, w.grad.view(GH, -1), accumulate=True)
      bias_grad_from_rows(d2, self.bx)
      if self.bh is not None:
        bias_grad_from_rows(dgr.view(B * T, GH), self.bh)
      # dWh += dgr^T . h_{t-1}: h_{t-1} is y shifted by one step in processing order
      if B * T >= SHIFTED_WH_MIN_ROWS and H % 8 == 0 and T > 1:
        # as a plain TN GEMM over a shifted copy of y (the 256 x 256 ping-pong weight-gradient kernel:
        # 165 -> ~90 us per DeepSpeech2 layer and direction) instead of the shifted-window K = 1 convolution
        # gradient on the lockstep tile. Rows at or past a sample's length carry zero gate gradients, and
        # y is zero there (the step kernels never write a finished sample), so the copy needs no mask.
        ysh = torch.empty((B, T, H), dtype=y.dtype, device=y.device)
        if self.reverse:
          ysh[:, :-1] = y[:, 1:]
          ysh[:, -1] = 0
        else:
          ysh[:, 1:] = y[:, :-1]
          ysh[:, 0] = 0
        capi.gemm_wgrad(ysh.view(B * T, H), dgr.view(B * T, GH), self.wh.grad.view(GH, H), accumulate=True)
      else:
        capi.conv1d_wgrad(y, dgr, 1, pad_left=(-1 if self.reverse else 1), in_len=lens,
                          out=self.wh.grad, accumulate=True)

  def forward(self, xs, lens, tape, y_view=None, dy_view_fn=None):
    """xs: list of Act [B,T,In_i]; lens int32 [B] or None. Returns Act [B,T,H].
    y_view: optional [B,T,H] channel-slice view to write the outputs into;
    dy_view_fn() then returns the matching slice of the shared gradient."""
    return rnn_directions_forward([self], xs, lens, tape, [y_view],
                                  [dy_view_fn] if dy_view_fn is not None else None)[0]


def rnn_directions_forward(dirs, xs, lens, tape, y_views=None, dy_view_fns=None, zoneout=None):
  """Runs 1 or 2 `RNNDirection`s of the same cell/size with ONE kernel launch per time step
  (os2s_rnn_layer_{fwd,bwd}_multi). `xs` is a list of Act shared by the directions, or one
  such list per direction. Returns one Act per direction.
  zoneout: dict(prob, mode, seeds_h, seeds_c) with one seed per direction (ZoneoutWrapper around each
  direction's cell, lstm_tf only; capi.ZONEOUT_SAMPLE when training, capi.ZONEOUT_BLEND otherwise)."""
  d0 = dirs[0]
  H = d0.H
  training = tape is not None
  y_views = y_views or [None] * len(dirs)
  xs_per = xs if isinstance(xs[0], (list, tuple)) else [xs] * len(dirs)
  gxs = [d.input_projection(x) for d, x in zip(dirs, xs_per)]
  res = capi.rnn_layer_fwd_multi(
      d0.cell, [dict(gx=gx, wh=d.wh.w16.view(d.G * H, H),
                     bh=d.bh.master if d.bh is not None else None, y=yv, reverse=d.reverse)
                for d, gx, yv in zip(dirs, gxs, y_views)],
      lens, H, d0.forget_bias, save=training, zoneout=zoneout)
  outs = [Act(r[0], lens) for r in res]
  if not training:
    return outs

  def backward():
    dys = [f() for f in dy_view_fns] if dy_view_fns is not None else [o.grad for o in outs]
    assert all(g is not None for g in dys)
    grads = capi.rnn_layer_bwd_multi(
        d0.cell, [dict(whT=d.wh.wt16.view(H, d.G * H), dy=dy, y=r[0], gates=r[1], c_seq=r[2],
                       reverse=d.reverse) for d, dy, r in zip(dirs, dys, res)],
        lens, H, d0.forget_bias, zoneout=zoneout)
    for d, x, r, (dgx, dgr) in zip(dirs, xs_per, res, grads):
      d.weight_backward(x, lens, r[0], dgx, dgr, h_seq=r[3] if zoneout is not None else None)
    for o in outs:
      o.grad = None

  tape.record(backward, [p for d in dirs for p in d.params()])
  return outs


class BiRNNStack(object):
  """num_layers x (forward + backward direction). The two directions of a layer write the two
  halves of ONE [B,T,2H] tensor (no concat), which the next layer / the following dense
  layer consumes as a single input (cuDNN 'bidirectional' stacking;
  tf.bidirectional_dynamic_rnn + tf.concat, ds2_encoder.py:294-380). Optional dropout between
  layers (cuDNN RNN `dropout`)."""

  def __init__(self, store, name, cell, input_size, hidden, num_layers, bidirectional=True,
               forget_bias=1.0):
    self.layers = []
    self.H, self.ndir = hidden, 2 if bidirectional else 1
    # the input GEMMs need a width that is a multiple of 8: a narrower input (13 MFCCs straight into the first
    # layer) is zero-padded in forward(), and the first layer's input kernels carry the logical width
    self.input_size, self.input_pad = input_size, -input_size % 8
    in_size = input_size + self.input_pad
    for l in range(num_layers):
      logical = input_size if (l == 0 and self.input_pad) else None
      dirs = [RNNDirection(store, "%s/layer_%d/fw" % (name, l), cell, [in_size], hidden, False,
                           forget_bias, logical_in=logical)]
      if bidirectional:
        dirs.append(RNNDirection(store, "%s/layer_%d/bw" % (name, l), cell, [in_size], hidden,
                                 True, forget_bias, logical_in=logical))
      self.layers.append(dirs)
      in_size = hidden * self.ndir
    self.output_dim = in_size

  def _padded(self, x, tape):
    """x [B,T,In] with zero columns up to the next multiple of 8 (the first layer's kernels are zero there)."""
    n = self.input_size
    wide = Act(torch.nn.functional.pad(x.data, (0, self.input_pad)), x.lens, requires_grad=x.requires_grad)
    if tape is not None and x.requires_grad:
      def backward():
        g = x.grad_buffer()
        if x.grad_init:
          g += wide.grad[:, :, :n]
        else:
          g.copy_(wide.grad[:, :, :n])
        x.grad_init = True
        wide.grad = None

      tape.record(backward)
    return wide

  def forward(self, x, lens, tape, keep_prob=1.0, seeds=None):
    """x: Act [B,T,In] -> Act [B,T,ndir*H]."""
    H = self.H
    cur = self._padded(x, tape) if self.input_pad else x
    for li, dirs in enumerate(self.layers):
      B, T, _ = cur.data.shape
      ybuf = (torch.zeros if lens is not None else torch.empty)(
          (B, T, H * self.ndir), dtype=torch.bfloat16, device=cur.data.device)
      out = Act(ybuf, lens)
      rnn_directions_forward(
          dirs, [cur], lens, tape, [ybuf[:, :, d * H:(d + 1) * H] for d in range(len(dirs))],
          [(lambda o=out, d=d: o.grad[:, :, d * H:(d + 1) * H]) for d in range(len(dirs))])
      cur = out
      if keep_prob < 1.0 and li < len(self.layers) - 1:
        seed = seeds.next() if seeds is not None else li + 1
        dropped = Act(capi.dropout_bwd(cur.data.view(-1, cur.data.shape[-1]), keep_prob,
                                       seed=seed).view_as(cur.data), lens)
        if tape is not None:
          src = cur

          def backward(dropped=dropped, src=src, seed=seed):
            g = capi.dropout_bwd(dropped.grad.view(-1, dropped.grad.shape[-1]), keep_prob,
                                 seed=seed).view_as(dropped.grad)
            src.grad, src.grad_init = g, True
            dropped.grad = None

          tape.record(backward)
        cur = dropped
    return cur


LN_SCOPES = ("input", "transform", "forget", "output", "state")     # the rows of the kernel's ln [10, H], in pairs


class LNLSTMLayer(object):
  """One layer of WeightDropLayerNormBasicLSTMCell with layer_norm=True (parts/rnns/weight_drop.py:140-166) under
  dynamic_rnn: no bias, LayerNorm (gamma init norm_gain, beta init norm_shift) on the four gate pre-activations
  and on the new cell state, recurrent dropout on the candidate. The input projection of all time steps is one
  GEMM, the recurrence is os2s_lnlstm_layer_fwd / _bwd (csrc/lnlstm.hip), the weight gradients are GEMMs over the
  saved gate gradients on the side stream (h_{t-1}: y shifted by one step, h0 in front)."""

  def __init__(self, store, name, input_size, hidden, forget_bias=1.0, norm_gain=1.0, norm_shift=0.0):
    self.H, self.input_size, self.forget_bias = hidden, input_size, float(forget_bias)
    GH = 4 * hidden
    if hidden % 8 or not 8 <= hidden <= 2048 or input_size % 8:
      raise NotImplementedError("LayerNorm-LSTM: num_units %d / input width %d (multiples of 8, units 8 .. 2048)"
                                % (hidden, input_size))

    def init(shape):    # glorot-uniform over the reference's one [in + H, 4H] kernel
      lim = math.sqrt(6.0 / (input_size + hidden + GH))
      return (torch.rand(shape) * 2 - 1) * lim

    self.wx = store.add(name + "/wx_0", (1, GH, input_size), init, kind="conv")
    self.wh = store.add(name + "/wh", (1, GH, hidden), init, kind="conv")
    self.ln = []
    for scope in LN_SCOPES:
      self.ln.append(store.add("%s/%s/gamma" % (name, scope), (hidden,), torch.full((hidden,), float(norm_gain)),
                               kind="vector"))
      self.ln.append(store.add("%s/%s/beta" % (name, scope), (hidden,), torch.full((hidden,), float(norm_shift)),
                               kind="vector"))

  def params(self):
    return [self.wx, self.wh] + self.ln

  def forward(self, x, lens, tape, keep_prob=1.0, seed=0, h0=None, c0=None, want_state=False, state_grad=None):
    """x: Act [B,T,In]; lens int32 [B] | None; h0 / c0 fp32 [B,H] | None. Returns Act [B,T,H], or (Act, hT, cT)
    with want_state. keep_prob: recurrent_keep_prob (the caller passes 1.0 outside training). state_grad: a dict
    that the consumer of hT / cT fills with 'dhT' / 'dcT' (fp32 [B,H]) in its own backward closure, which runs
    before this layer's; the backward is then os2s_lnlstm_layer_bwd_state and the gradient of y may be absent."""
    B, T, _ = x.data.shape
    H, GH = self.H, 4 * self.H
    x2 = x.data.reshape(B * T, -1)
    gx = capi.gemm(x2, self.wx.w16.view(GH, -1)).view(B, T, GH)
    ln = torch.stack([p.master for p in self.ln])
    r = capi.lnlstm_layer_fwd(gx, self.wh.w16.view(GH, H), ln, lens, H, self.forget_bias, keep_prob, seed, h0, c0,
                              save=tape is not None, want_state=want_state)
    out = Act(r["y"], lens)
    if tape is not None:
      layer = self

      def backward():
        if state_grad is not None:
          assert out.grad is not None or state_grad.get("dhT") is not None or state_grad.get("dcT") is not None, \
              "no gradient reached " + layer.wh.name
          dgx, dln = capi.lnlstm_layer_bwd_state(layer.wh.wt16.view(H, GH), ln, lens, out.grad, state_grad.get("dhT"),
                                                 state_grad.get("dcT"), r["xhat"], r["s_hat"], r["rstd"], H,
                                                 layer.forget_bias, keep_prob, seed, c0)
          state_grad.clear()
        else:
          assert out.grad is not None, "no gradient reached " + layer.wh.name
          dgx, dln = capi.lnlstm_layer_bwd(layer.wh.wt16.view(H, GH), ln, lens, out.grad, r["xhat"], r["s_hat"],
                                           r["rstd"], H, layer.forget_bias, keep_prob, seed, c0)
        d2 = dgx.view(B * T, GH)
        if x.requires_grad:
          g = x.grad_buffer()
          capi.gemm(d2, layer.wx.wt16.view(-1, GH), out=g.view(B * T, -1), accumulate=x.grad_init)
          x.grad_init = True
        for k, p in enumerate(layer.ln):
          p.grad.add_(dln[k])
        with on_side_stream(dgx.device, dgx, r["y"], x.data, *([h0] if h0 is not None else [])):
          capi.gemm_wgrad(x2, d2, layer.wx.grad.view(GH, -1), accumulate=True)
          # dWh += dgx^T . h_{t-1}. Rows at or past a sample's length carry zero gate gradients
          ysh = torch.empty((B, T, H), dtype=r["y"].dtype, device=dgx.device)
          ysh[:, 1:] = r["y"][:, :-1]
          if h0 is not None:
            ysh[:, 0] = h0.to(ysh.dtype)
          else:
            ysh[:, 0] = 0
          capi.gemm_wgrad(ysh.view(B * T, H), d2, layer.wh.grad.view(GH, H), accumulate=True)
        out.grad = None

      tape.record(backward, self.params())
    return (out, r["hT"], r["cT"]) if want_state else out

  def step(self, x2d, h, c):
    """One generation step without dropout: x2d bf16 [B,In], h / c fp32 [B,H] | None -> (y bf16 [B,H], h', c')."""
    out, h, c = self.forward(Act(x2d.view(x2d.shape[0], 1, -1), requires_grad=False), None, None, h0=h, c0=c,
                             want_state=True)
    return out.data.view(x2d.shape[0], self.H), h, c
