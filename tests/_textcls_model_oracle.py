"""Helper of tests/test_ref_exec_textcls.py and tests/test_ref_exec_textcls_gpu.py (not a test module): the
text-classification network of tests/golden/ref_exec_textcls.npz (EncoderEmbeddingMatrix -> LayerNorm-LSTM layers
under sequence lengths -> the last layer's final state h or [h, c] -> Dense -> softmax cross-entropy summed over
the classes and divided by B) restated on the oracles of tests/_lnlstm_cases.py and tests/_textcls_cases.py,
forward and backward by hand, in the reference's variable names and layouts (those of tests/_lm_model_oracle.py).

rounded=False is R. rounded=True is R_b: a bf16 round where the device stores bf16 — the bf16 compute copies of the
matrices (embedding table, cell kernels, dense kernel), the hoisted input projection gx, the recurrence's own
stores (see _lnlstm_cases), dgx and the data gradient handed to the layer below. The final state, the logits, the
loss, the logits gradient, dhT / dcT, the LayerNorm parameters, the bias and every weight-gradient accumulation
stay fp32 on the device, unrounded here. dtype=torch.float32 (unrounded) gives the round-off scale of an fp32
evaluation such as the fixture's."""
import numpy as np
import torch

import _lnlstm_cases as C
import _textcls_cases as X
from _lm_model_oracle import CELL, LN, SCOPE


def run(var, src, lens, labels, n_layers, use_cell_state, rounded=False, dtype=torch.float64):
  """var: {reference name: array}. Returns dict(logits [B,C], loss, grads {reference name: tensor})."""
  rd = C.rb if rounded else (lambda x: x)
  t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
  src = torch.as_tensor(np.asarray(src)).long()
  lens = torch.as_tensor(np.asarray(lens)).to(torch.int32)
  y = t(labels)
  B, T = src.shape
  table = rd(t(var[SCOPE + "/EncoderEmbeddingMatrix"]))      # [V, E]
  W = rd(t(var[SCOPE + "/dense/kernel"]).t())                # [C, D]
  bias = t(var[SCOPE + "/dense/bias"])
  cur = table[src]
  layers = []
  for k in range(n_layers):
    K = t(var[(CELL % k) + "/kernel"])                       # [in + H, 4H], input rows first
    n_in = cur.shape[2]
    Wx, Wh = rd(K[:n_in].t()), rd(K[n_in:].t())
    ln = torch.stack([t(var["%s/%s/%s" % (CELL % k, s, g)]) for s in LN for g in ("gamma", "beta")])
    gx = rd(cur @ Wx.t())
    fw = C.forward_oracle(gx, Wh, ln, lens, rounded=rounded, dtype=dtype)
    layers.append((cur, Wx, Wh, ln, fw))
    cur = fw["y"]
  top = layers[-1][4]
  s = torch.cat([top["hT"], top["cT"]], dim=1) if use_cell_state else top["hT"]
  logits = s @ W.t() + bias
  logp = torch.log_softmax(logits, dim=1)
  loss = -(logp * y).sum() / B
  dl = (torch.exp(logp) * y.sum(1, keepdim=True) - y) / B
  grads = {SCOPE + "/dense/bias": dl.sum(0), SCOPE + "/dense/kernel": (dl.t() @ s).t()}
  ds = dl @ W
  H_top = top["hT"].shape[1]
  dhT, dcT = ds[:, :H_top], (ds[:, H_top:] if use_cell_state else None)
  dcur = None
  for k in range(n_layers - 1, -1, -1):
    x, Wx, Wh, ln, fw = layers[k]
    if k == n_layers - 1:
      bw = X.backward_state_oracle(fw["xhat"], fw["s_hat"], fw["rstd"], None, dhT, dcT, Wh, ln, lens, rounded=rounded,
                                   dtype=dtype)
    else:
      bw = C.backward_oracle(fw["xhat"], fw["s_hat"], fw["rstd"], dcur, Wh, ln, lens, rounded=rounded, dtype=dtype)
    d2 = bw["dgx"].reshape(B * T, -1)
    hprev = torch.cat([torch.zeros_like(fw["y"][:, :1]), fw["y"][:, :-1]], dim=1)
    grads[(CELL % k) + "/kernel"] = torch.cat([x.reshape(B * T, -1).t() @ d2, hprev.reshape(B * T, -1).t() @ d2], dim=0)
    for i, sc in enumerate(LN):
      grads["%s/%s/gamma" % (CELL % k, sc)] = bw["dln"][2 * i]
      grads["%s/%s/beta" % (CELL % k, sc)] = bw["dln"][2 * i + 1]
    dcur = rd(d2 @ Wx).view(B, T, -1)
  grads[SCOPE + "/EncoderEmbeddingMatrix"] = torch.zeros_like(table).index_add(0, src.reshape(-1),
                                                                              dcur.reshape(B * T, -1))
  return dict(logits=logits, loss=loss, grads=grads)
