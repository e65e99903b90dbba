"""os2s_xent_smooth above V = 40960 (the streamed kernel: the word-level vocabularies of the language models' eval)
against the fp64 expression tests/test_transformer_kernels_gpu.py::test_xent_smooth uses (soft targets 1 - s at the
label, s / (V_valid - 1) elsewhere, minus the smoothing constant; here with vocabulary padding columns and a masked
row), at that test's tolerance. V = 40960 still takes the register-resident kernel: its row losses and gradient are
bit-identical to what the commit before the streamed kernel gave for the same input, recorded as SHA-256 digests in
tests/golden/xent_smooth_v40960.json."""
import hashlib
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xent_smooth_v40960.json")


def _inputs(V, v_valid, seed):
  g = torch.Generator().manual_seed(seed)
  N = 3
  logits = (torch.randn(N, V, generator=g) * 3).to(torch.bfloat16)
  labels = torch.randint(0, v_valid, (N,), generator=g).to(torch.int32)
  labels[1] = -1                                  # one masked row
  return logits, labels


def _fp64(logits, labels, v_valid, smoothing):
  """(mean over the N rows, d mean / d logits): the oracle's padded_xent_smoothing in fp64 over the first v_valid
  columns; a row with label < 0 has weight 0."""
  lf = logits.double().requires_grad_(True)
  conf = 1.0 - smoothing
  low = (1.0 - conf) / float(v_valid - 1)
  live = labels >= 0
  soft = torch.full((logits.shape[0], v_valid), low, dtype=torch.float64)
  soft.scatter_(-1, labels.clamp(min=0).long()[:, None], conf)
  xent = -(soft * torch.log_softmax(lf[:, :v_valid], -1)).sum(-1)
  norm = -((conf * math.log(conf) if conf > 0 else 0.0) + float(v_valid - 1) * low * math.log(low + 1e-20))
  mean = ((xent - norm) * live.double()).sum() / logits.shape[0]
  mean.backward()
  return mean.detach(), lf.grad


@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("V,v_valid", [(40968, 40961), (65536, 65536)])
def test_streamed_xent_against_fp64(cuda, V, v_valid, smoothing, want_grad):
  from openseq2seq_amd import capi
  logits, labels = _inputs(V, v_valid, seed=V)
  rl, mean, dl = capi.xent_smooth(logits.to(cuda), labels.to(cuda), smoothing, want_grad=want_grad, v_valid=v_valid)
  torch.cuda.synchronize()
  ref, gref = _fp64(logits, labels, v_valid, smoothing)
  torch.testing.assert_close(mean.cpu()[0].double(), ref, rtol=2e-3, atol=2e-3)
  assert float(rl[1]) == 0.0
  if not want_grad:
    assert dl is None
    return
  err = (dl.double().cpu() - gref).abs().max()
  assert float(err) < 2e-2 * float(gref.abs().max()) + 1e-6
  assert not dl[1].any() and not dl[:, v_valid:].any()      # masked row, vocabulary padding


def golden_digests(device):
  """SHA-256 of row_loss and dlogits bytes of the V = 40960 case (also run from the commit before this kernel to
  record the fixture)."""
  from openseq2seq_amd import capi
  out = {}
  for smoothing in (0.0, 0.1):
    logits, labels = _inputs(40960, 40955, seed=40960)
    rl, mean, dl = capi.xent_smooth(logits.to(device), labels.to(device), smoothing, v_valid=40955)
    torch.cuda.synchronize()
    for name, t in (("row_loss", rl), ("loss", mean), ("dlogits", dl)):
      out["%s_s%.1f" % (name, smoothing)] = hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
  return out


def test_v40960_keeps_the_register_kernel_bit_for_bit(cuda):
  want = json.load(open(GOLDEN))
  assert golden_digests(cuda) == want["sha256"]
