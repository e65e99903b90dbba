"""The final-state classification head (csrc/text_cls.hip: os2s_text_cls_fwd, os2s_softmax_xent_dense,
os2s_text_cls_bwd) against the float64 oracle of tests/_textcls_cases.py, whose docstring lists the cases, what
each makes the kernels do, and derives the bound: every output is an fp32 sum and holds the running-error bound
|got - R| <= n 2^-23 S elementwise (S the oracle's sum of the absolute values of the element's terms, n their
number, + 8 for the loss kernel's exp / log), stage by stage on the device's output of the stage before. Weights
are bf16-representable, states and labels fp32 with one soft label row, the loss scale 1 and 1024. Exact: a rerun
is bit-identical, want_grad=False writes no gradient and the same loss, C or H out of contract are refused."""
import pytest
import torch

import _lnlstm_cases as C
import _textcls_cases as X


@pytest.mark.gpu
@pytest.mark.parametrize("scale", X.SCALES)
@pytest.mark.parametrize("case", list(X.HEAD_CASES))
def test_text_cls_head(cuda, case, scale):
  got = X.run_head_gpu(case, scale, cuda)
  fails = X.check_head(case, scale, got)
  again = X.run_head_gpu(case, scale, cuda)
  for q, t in got.items():
    if t is not None and not C.same_bits(t, again[q]):
      fails.append("%s: %s not bit-identical on a rerun" % (case, q))
  nograd = X.run_head_gpu(case, scale, cuda, want_grad=False)
  if nograd["dlogits"] is not None or not C.same_bits(nograd["loss"], got["loss"]):
    fails.append("%s: want_grad=False" % case)
  assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_text_cls_contract(cuda):
  from openseq2seq_amd import _lib, capi

  def call(B, H, Cn):
    h = torch.zeros((B, H), dtype=torch.float32, device=cuda)
    w = torch.zeros((Cn, H), dtype=torch.bfloat16, device=cuda)
    return capi.text_cls_fwd(h, None, w, None)

  assert tuple(call(2, 16, 16).shape) == (2, 16)
  for H, Cn in ((12, 2), (2056, 2), (16, 1), (16, 17)):
    with pytest.raises(_lib.Os2sError):
      call(1, H, Cn)
    with pytest.raises(_lib.Os2sError):
      h = torch.zeros((1, H), dtype=torch.float32, device=cuda)
      capi.text_cls_bwd(h, None, torch.zeros((Cn, H), dtype=torch.bfloat16, device=cuda),
                        torch.zeros((1, Cn), dtype=torch.float32, device=cuda),
                        torch.zeros((Cn, H), dtype=torch.float32, device=cuda), None)
  for Cn in (1, 17):
    z = torch.zeros((1, Cn), dtype=torch.float32, device=cuda)
    with pytest.raises(_lib.Os2sError):
      capi.softmax_xent_dense(z, z)
