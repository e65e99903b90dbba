"""Every kernel instance of the LayerNorm-LSTM recurrence (csrc/lnlstm.hip) against the float64 oracle of
tests/_lnlstm_cases.py, whose docstring lists the instance each case reaches and states the bound:
|got - R_b| <= 4 n_q + 2^-7 |R_b| elementwise on y, the saved xhat / s_hat / rstd, hT, cT, dgx and the ten
LayerNorm parameter gradients (dln), n_q computed from the oracle alone. Exact: zeros past the lengths,
untouched guard columns in the strided run, a rerun bit-identical (dln included), the keep mask equal to
capi.dropout_mask at the same seed and indices, and, without dropout, a T-step call equal to T one-step calls
chained through h0 / c0 -> hT / cT bit for bit. tests/test_lnlstm_oracle_cpu.py shows on the CPU that the bound
rejects eight wrong recurrences and holds the backward oracle against autograd."""
import pytest

import _lnlstm_cases as C


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(C.CASES))
def test_lnlstm_paths(cuda, case):
  fails = C.check_case(case, cuda)
  assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_lnlstm_shape_contract(cuda):
  """Outside H % 8 == 0, 8 <= H <= 2048 the entry points refuse with OS2S_ERR_UNSUPPORTED instead of running."""
  import torch
  from openseq2seq_amd import _lib, capi
  for H in (12, 2056):
    gx = torch.zeros((1, 1, 4 * H), dtype=torch.bfloat16, device=cuda)
    wh = torch.zeros((4 * H, H), dtype=torch.bfloat16, device=cuda)
    ln = torch.zeros((10, H), dtype=torch.float32, device=cuda)
    with pytest.raises(_lib.Os2sError):
      capi.lnlstm_layer_fwd(gx, wh, ln, None, H)
