"""Helper of tests/test_ref_exec_lm.py and tests/test_ref_exec_lm_gpu.py (not a test module): the LSTM language
model of tests/golden/ref_exec_lm.npz (weight-tied embedding -> LayerNorm-LSTM layers -> Dense logits ->
BasicSequenceLoss averaged over all B x T entries) restated on the recurrence oracle of tests/_lnlstm_cases.py,
forward and backward by hand, in the reference's variable names and layouts.

rounded=False is R. rounded=True is R_b: a bf16 round where the device stores bf16 — the bf16 compute copies of the
matrices (dense kernel = embedding table, cell kernels), the hoisted input projection gx, the recurrence's own
stores (see _lnlstm_cases), the logits, the logits gradient, dgx and the data gradient handed to the layer below.
LayerNorm parameters, the bias and every weight-gradient accumulation stay fp32 on the device, unrounded here.
dtype=torch.float32 (unrounded) gives the round-off scale of an fp32 evaluation such as the fixture's."""
import numpy as np
import torch

import _lnlstm_cases as C

SCOPE = "ForwardPass/rnn_encoder_awd"
CELL = SCOPE + "/decoder/multi_rnn_cell/cell_%d/weight_drop_layer_norm_basic_lstm_cell"
LN = ("input", "transform", "forget", "output", "state")


def run(var, src, tgt, n_layers, rounded=False, dtype=torch.float64):
  """var: {reference name: array}. Returns dict(logits [B,T,V], loss, grads {reference name: tensor})."""
  rd = C.rb if rounded else (lambda x: x)
  t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
  src, tgt = torch.as_tensor(np.asarray(src)).long(), torch.as_tensor(np.asarray(tgt)).long()
  B, T = src.shape
  P = rd(t(var[SCOPE + "/dense/kernel"]).t())               # [V, E]: the output layer's rows = the embedding table
  bias = t(var[SCOPE + "/dense/bias"])
  V = P.shape[0]
  cur = P[src]
  layers = []
  for k in range(n_layers):
    K = t(var[(CELL % k) + "/kernel"])                       # [in + H, 4H], input rows first
    n_in = cur.shape[2]
    Wx, Wh = rd(K[:n_in].t()), rd(K[n_in:].t())
    ln = torch.stack([t(var["%s/%s/%s" % (CELL % k, s, g)]) for s in LN for g in ("gamma", "beta")])
    gx = rd(cur @ Wx.t())
    fw = C.forward_oracle(gx, Wh, ln, None, rounded=rounded, dtype=dtype)
    layers.append((cur, Wx, Wh, ln, fw))
    cur = fw["y"]
  logits = rd(cur @ P.t() + bias)
  logp = torch.log_softmax(logits, dim=2)
  onehot = torch.nn.functional.one_hot(tgt, V).to(dtype)
  loss = -(logp * onehot).sum() / (B * T)
  dl = rd((torch.exp(logp) - onehot) / (B * T)).reshape(B * T, V)
  grads = {SCOPE + "/dense/bias": dl.sum(0)}
  dP = dl.t() @ cur.reshape(B * T, -1)
  dcur = rd(dl @ P).view(B, T, -1)
  for k in range(n_layers - 1, -1, -1):
    x, Wx, Wh, ln, fw = layers[k]
    bw = C.backward_oracle(fw["xhat"], fw["s_hat"], fw["rstd"], dcur, Wh, ln, None, rounded=rounded, dtype=dtype)
    d2 = bw["dgx"].reshape(B * T, -1)
    hprev = torch.cat([torch.zeros_like(fw["y"][:, :1]), fw["y"][:, :-1]], dim=1)
    dK = torch.cat([x.reshape(B * T, -1).t() @ d2, hprev.reshape(B * T, -1).t() @ d2], dim=0)
    grads[(CELL % k) + "/kernel"] = dK
    for i, s in enumerate(LN):
      grads["%s/%s/gamma" % (CELL % k, s)] = bw["dln"][2 * i]
      grads["%s/%s/beta" % (CELL % k, s)] = bw["dln"][2 * i + 1]
    dcur = rd(d2 @ Wx).view(B, T, -1)
  dP = dP.index_add(0, src.reshape(-1), dcur.reshape(B * T, -1))
  grads[SCOPE + "/dense/kernel"] = dP.t()
  return dict(logits=logits, loss=loss, grads=grads)
