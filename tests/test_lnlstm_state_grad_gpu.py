"""os2s_lnlstm_layer_bwd_state (csrc/lnlstm.hip): the LayerNorm-LSTM backward with a gradient on the final
state, against the float64 oracle of tests/_textcls_cases.py on the geometries of _lnlstm_cases.CASES that reach
cb<1>, cb<2>, cb<4> and both batch tiles. Per case four gradient mixes (dy = NULL with dhT + dcT; dy + dhT + dcT;
dhT alone; dy + dcT, which runs the plain cell instance); dgx and dln hold |got - R_b| <= 4 n_q + 2^-7 |R_b|, the
backward teacher-forced on the device's own saved tensors and n_q from the oracle alone. Exact: rows at or past a length (a length-0 sample's rows among them)
are zero, dy = NULL equals dy = zeros, dhT = dcT = NULL equals os2s_lnlstm_layer_bwd, a rerun is bit-identical.
tests/test_textcls_oracle_cpu.py holds the oracle against autograd and shows that the bound rejects a state
gradient entered at T - 1, a dropped dcT and a dcT that skips the state LayerNorm."""
import pytest
import torch

import _lnlstm_cases as C
import _textcls_cases as X


@pytest.mark.gpu
@pytest.mark.parametrize("case", X.STATE_CASES)
def test_lnlstm_state_grad(cuda, case):
  from openseq2seq_amd import capi
  s = C.spec(case)
  d = C.build_inputs(case)
  fw, out, extras = X.run_state_gpu(case, cuda)
  saved = {k: fw[k].cpu() for k in ("xhat", "s_hat", "rstd")}
  mask = None
  if d["keep"] < 1.0:
    mask = capi.dropout_mask(d["seed"], s["B"] * s["T"] * s["H"], d["keep"], cuda).cpu().view(s["B"], s["T"], s["H"])
  fails = []
  dead = ~C.live_steps(case)
  for mix in X.MIXES:
    ref = X.reference_state_bwd(case, mix, saved, True, mask)
    for q, ok, err, ratio in C.within(case, out[mix], ref, X.state_noise_floor(case, mix), log=print):
      if not ok:
        fails.append("%s/%s: %s max err %.3e, err/bound %.3e" % (case, mix, q, err, ratio))
    assert float(out[mix]["dgx"].double().abs().max()) > 0.0
    if bool(dead.any()) and not bool((out[mix]["dgx"].double()[dead] == 0.0).all()):
      fails.append("%s/%s: dgx rows of finished steps not zero" % (case, mix))
  lens = d["lens"]
  if lens is not None and bool((lens <= 0).any()):
    empty = (lens <= 0).nonzero().flatten()
    for mix in X.MIXES:
      if not bool((out[mix]["dgx"][empty].double() == 0.0).all()):
        fails.append("%s/%s: a length-0 sample has gate gradients" % (case, mix))
  for a, b, what in ((out["state_only"], extras["zeros_dy"], "dy = NULL vs dy = zeros"),
                     (extras["state_null"], extras["plain"], "dhT = dcT = NULL vs os2s_lnlstm_layer_bwd"),
                     (out["all"], extras["again"], "rerun")):
    for q in C.BWD_OUT:
      if not C.same_bits(a[q], b[q]):
        fails.append("%s: %s not bit-identical (%s)" % (case, q, what))
  assert not fails, "\n".join(fails)
