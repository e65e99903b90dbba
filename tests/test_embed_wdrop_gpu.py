"""Embedding lookup with dropout on the matrix (os2s_embed_wdrop_fwd / _bwd, encoders/lm_encoders.py:264): V = 19,
E = 8, ids with repeats, keep 0.37. The forward equals the gather of table * mask / keep with the mask read back
through capi.dropout_mask at (seed, id E + column), bit for bit; repeated ids share their mask; the backward
equals the float64 scatter-add of dout * mask / keep within bf16 round-off of the sum of the magnitudes (the
device accumulates in fp32, far inside it), with atomics and in deterministic mode."""
import pytest
import torch

V, E, KEEP, SEED = 19, 8, 0.37, 0xabcdef12345
IDS = [3, 18, 0, 3, 7, 18, 18, 5, 0, 3, 11, 12]


def _inputs(dev):
  g = torch.Generator().manual_seed(5)
  table = torch.randn(V, E, generator=g).to(torch.bfloat16)
  dout = torch.randn(len(IDS), E, generator=g).to(torch.bfloat16)
  return table.to(dev), dout.to(dev), torch.tensor(IDS, dtype=torch.int32, device=dev)


@pytest.mark.gpu
def test_embed_wdrop_forward(cuda):
  from openseq2seq_amd import capi
  table, _, ids = _inputs(cuda)
  mask = capi.dropout_mask(SEED, V * E, KEEP, cuda).view(V, E)
  frac = float(mask.float().mean())
  assert 0.2 < frac < 0.55, frac
  out = capi.embed_wdrop_fwd(ids, table, KEEP, SEED)
  ik = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(KEEP, dtype=torch.float32)
  dropped = torch.where(mask, table.float() * ik.to(cuda), torch.zeros((), device=cuda)).to(torch.bfloat16)
  assert torch.equal(out.view(torch.int16), dropped[ids.long()].view(torch.int16))
  for a in range(len(IDS)):
    for b in range(a + 1, len(IDS)):
      if IDS[a] == IDS[b]:
        assert torch.equal(out[a].view(torch.int16), out[b].view(torch.int16))
  # keep = 1: the plain lookup
  assert torch.equal(capi.embed_wdrop_fwd(ids, table, 1.0, SEED).view(torch.int16), table[ids.long()].view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("deterministic", [False, True])
def test_embed_wdrop_backward(cuda, deterministic):
  from openseq2seq_amd import capi
  _, dout, ids = _inputs(cuda)
  mask = capi.dropout_mask(SEED, V * E, KEEP, cuda).view(V, E).cpu()
  ref = torch.zeros(V, E, dtype=torch.float64)
  mag = torch.zeros(V, E, dtype=torch.float64)
  d64 = dout.cpu().double()
  for n, i in enumerate(IDS):
    ref[i] += d64[n] * mask[i].double() / KEEP
    mag[i] += (d64[n] * mask[i].double() / KEEP).abs()
  dtable = torch.zeros(V, E, dtype=torch.float32, device=cuda)
  was = capi.deterministic()
  capi.set_deterministic(deterministic)
  try:
    capi.embed_wdrop_bwd(ids, dout, dtable, KEEP, SEED)
    torch.cuda.synchronize()
  finally:
    capi.set_deterministic(was)
  got = dtable.cpu().double()
  assert bool(((got - ref).abs() <= 2.0 ** -9 * mag).all()), float((got - ref).abs().max())
  untouched = torch.ones(V, dtype=torch.bool)
  untouched[torch.tensor(IDS)] = False
  assert bool((got[untouched] == 0).all()) and bool((got[~mask] == 0).all())
  assert float(ref.abs().max()) > 0.0
