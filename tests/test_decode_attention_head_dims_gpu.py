"""Incremental decode attention (csrc/decode_attention.hip) at head dims 8, 16, 32 and 128 against a float64
single-query oracle: the self-attention kernel (cache append, ancestry table) and the encoder-decoder kernel.
N = 6 rows (2 sentences x beam 3), H = 3 heads, q / k / v as column slices; Tmax = 70 with steps on both sides
of the 64-key batch of the kernel's loop; a non-identity ancestry table. Outputs: 2e-2 of the rms (bf16 output);
the appended cache rows and the ancestry entry bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HEAD_DIMS = [8, 16, 32, 128]
N, H, TMAX = 6, 3, 70


def _close(got, ref, tol=2e-2):
  scale = float(ref.pow(2).mean().sqrt()) + 1e-8
  torch.testing.assert_close(got.double().cpu(), ref, rtol=tol, atol=tol * scale)


def _single_query(q, K, V, dh, scale):
  """q [D], K / V [T, D] float64 -> [D]"""
  s = torch.einsum("hd,thd->ht", q.view(H, dh), K.view(-1, H, dh)) * scale
  return torch.einsum("ht,thd->hd", torch.softmax(s, -1), V.view(-1, H, dh)).reshape(-1)


@pytest.mark.parametrize("step", [0, 1, 63, 64, 69])
@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_decode_self_attention_head_dims(cuda, dh, step):
  from openseq2seq_amd import capi
  D = H * dh
  g = torch.Generator().manual_seed(100 * dh + step)
  qkv = torch.randn(N, 3 * D, generator=g).to(torch.bfloat16).to(cuda)
  kc = torch.randn(N, TMAX, D, generator=g).to(torch.bfloat16).to(cuda)
  vc = torch.randn(N, TMAX, D, generator=g).to(torch.bfloat16).to(cuda)
  anc = torch.randint(0, N, (N, TMAX), generator=g, dtype=torch.int32).to(cuda)
  kc0, vc0, anc0 = kc.clone(), vc.clone(), anc.clone()
  scale = dh ** -0.5
  o = capi.decode_self_attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], kc, vc, anc, H, step, scale)
  torch.cuda.synchronize()
  # cache append + ancestry of the new slot, nothing else touched
  assert torch.equal(kc[:, step], qkv[:, D:2 * D]) and torch.equal(vc[:, step], qkv[:, 2 * D:])
  assert torch.equal(anc[:, step].cpu(), torch.arange(N, dtype=torch.int32))
  keep = torch.ones(TMAX, dtype=torch.bool)
  keep[step] = False
  assert torch.equal(kc[:, keep], kc0[:, keep]) and torch.equal(vc[:, keep], vc0[:, keep])
  assert torch.equal(anc[:, keep], anc0[:, keep])
  a = anc.long().cpu()
  kf, vf, qf = kc.double().cpu(), vc.double().cpu(), qkv[:, :D].double().cpu()
  pos = torch.arange(step + 1)
  ref = torch.stack([_single_query(qf[n], kf[a[n, :step + 1], pos], vf[a[n, :step + 1], pos], dh, scale)
                     for n in range(N)])
  _close(o, ref)


@pytest.mark.parametrize("lens", [[1, 9], [70, 9], [9, 70]])
@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_decode_cross_attention_head_dims(cuda, dh, lens):
  from openseq2seq_amd import capi
  beam = N // len(lens)
  D = H * dh
  cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
  g = torch.Generator().manual_seed(dh + lens[0])
  kv = torch.randn(int(cu[-1]), 2 * D, generator=g).to(torch.bfloat16).to(cuda)
  q = torch.randn(N, D, generator=g).to(torch.bfloat16).to(cuda)
  scale = dh ** -0.5
  o = capi.decode_cross_attention(q, kv[:, :D], kv[:, D:], cu.to(cuda), beam, H, max(lens), scale)
  torch.cuda.synchronize()
  kvf, qf = kv.double().cpu(), q.double().cpu()
  ref = torch.stack([_single_query(qf[n], kvf[cu[n // beam]:cu[n // beam + 1], :D].contiguous(),
                                   kvf[cu[n // beam]:cu[n // beam + 1], D:].contiguous(), dh, scale)
                     for n in range(N)])
  _close(o, ref)


@pytest.mark.parametrize("dh", [24, 256])
def test_decode_attention_unsupported_head_dim_raises(cuda, dh):
  from openseq2seq_amd import capi
  D = H * dh
  q = torch.zeros(N, D, dtype=torch.bfloat16, device=cuda)
  c = torch.zeros(N, 4, D, dtype=torch.bfloat16, device=cuda)
  anc = torch.zeros(N, 4, dtype=torch.int32, device=cuda)
  cu = torch.tensor([0, 3, 6], dtype=torch.int32, device=cuda)
  with pytest.raises(NotImplementedError, match="8, 16, 32, 64, 128"):
    capi.decode_self_attention(q, q, q, c, c, anc, H, 0, 1.0)
  with pytest.raises(NotImplementedError, match="8, 16, 32, 64, 128"):
    capi.decode_cross_attention(q, q, q, cu, 3, H, 3, 1.0)
