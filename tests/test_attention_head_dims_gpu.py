"""The attention kernels (csrc/attention.hip: attn_fwd_kernel / attn_bwd_kernel / attn_fwd_long_kernel<DH, kDrop>) at
every head dim they are instantiated for, 8, 16, 32, 64 and 128, against a float64 oracle:
the cases of test_attention_fwd_bwd / test_attention_fwd_long (tests/test_transformer_kernels_gpu.py) with that
file's bounds — o 2e-2 of the tensor rms, gradients 3e-2, lse 2e-3; long forward 2e-2 / 2e-3. bf16 I/O rounding
dominates at every head dim, so the bounds do not depend on it.

H = 3 heads and q / k / v passed as column slices of one [N, 3*H*dh] tensor: with dh < 64 a kernel that takes
64 channels per head reads the neighbouring head (or the next slice) as if it were its own. Outputs are
torch.empty buffers, so a dropped store shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HEAD_DIMS = [8, 16, 32, 64, 128]
B, H = 5, 3


def _close(got, ref, tol):
  got = got.double().cpu()
  scale = float(ref.pow(2).mean().sqrt()) + 1e-8
  torch.testing.assert_close(got, ref, rtol=tol, atol=tol * scale)


def _cu(lens, dev):
  return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)


def _inputs(g, lq, lk, D, cross, dev):
  """(q, k, v) device views with row stride 3 * D, and their float64 host copies."""
  if cross:
    qs = torch.randn(sum(lq), 3 * D, generator=g).to(torch.bfloat16).to(dev)
    ks = torch.randn(sum(lk), 3 * D, generator=g).to(torch.bfloat16).to(dev)
    q, k, v = qs[:, D:2 * D], ks[:, :D], ks[:, 2 * D:]
  else:
    qkv = torch.randn(sum(lq), 3 * D, generator=g).to(torch.bfloat16).to(dev)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
  assert q.stride(0) == 3 * D
  return (q, k, v), tuple(t.double().cpu().contiguous() for t in (q, k, v))


def _oracle(qf, kf, vf, lq, lk, dh, scale, causal, mask=None, keep=1.0):
  """float64 attention per packed sequence: (o [Nq, D], lse [Nq, H])."""
  outs, lses = [], []
  oq = ok = 0
  for b in range(len(lq)):
    Q = qf[oq:oq + lq[b]].view(lq[b], H, dh).transpose(0, 1)
    K = kf[ok:ok + lk[b]].view(lk[b], H, dh).transpose(0, 1)
    V = vf[ok:ok + lk[b]].view(lk[b], H, dh).transpose(0, 1)
    S = (Q * scale) @ K.transpose(-1, -2)
    if causal:
      S = S + torch.triu(torch.full((lq[b], lk[b]), float("-inf"), dtype=torch.float64), diagonal=1)
    P = torch.softmax(S, -1)
    lses.append(torch.logsumexp(S.detach(), -1).transpose(0, 1))
    if mask is not None:
      P = P * mask[b, :, :lq[b], :lk[b]].double() / keep
    outs.append((P @ V).transpose(0, 1).reshape(lq[b], H * dh))
    oq += lq[b]; ok += lk[b]
  return torch.cat(outs, 0), torch.cat(lses, 0)


@pytest.mark.parametrize("causal,cross", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("keep", [1.0, 0.9])
@pytest.mark.parametrize("lens", [([64, 17, 1, 33, 56], [40, 64, 9, 2, 56]),
                                  ([32, 16, 48, 31, 49], [16, 32, 33, 64, 15])])
@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_fwd_bwd_head_dims(cuda, dh, lens, keep, causal, cross):
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(7 + causal + 2 * cross + dh)
  D = H * dh
  lq = lens[0]
  lk = lens[1] if cross else lq
  (q, k, v), (qf, kf, vf) = _inputs(g, lq, lk, D, cross, cuda)
  do = torch.randn(sum(lq), D, generator=g).to(torch.bfloat16)
  scale = dh ** -0.5
  cq, ck = _cu(lq, cuda), _cu(lk, cuda)
  seed = 99
  o, lse = capi.attention_fwd(q, k, v, cq, ck, H, 64, causal, scale, keep, seed, dh=dh)
  # gradients into column slices too: the stores must stay inside each head's dh channels
  gq = torch.full((sum(lq), 3 * D), 7.0, dtype=torch.bfloat16, device=cuda)
  gk = torch.full((sum(lk), 3 * D), 7.0, dtype=torch.bfloat16, device=cuda)
  dq, dk, dv = gq[:, D:2 * D], gk[:, :D], gk[:, 2 * D:]
  capi.attention_bwd(q, k, v, do.to(cuda), lse, dq, dk, dv, cq, ck, H, 64, causal, scale, keep, seed, dh=dh)
  torch.cuda.synchronize()
  mask = None
  if keep < 1.0:      # the device mask: element ((b*H+h)*64 + q)*64 + key, whatever the head dim
    mask = capi.dropout_mask(seed, B * H * 64 * 64, keep, cuda).cpu().view(B, H, 64, 64)
  qf, kf, vf = (t.requires_grad_(True) for t in (qf, kf, vf))
  ref, lse_ref = _oracle(qf, kf, vf, lq, lk, dh, scale, causal, mask, keep)
  ref.backward(do.double())
  torch.testing.assert_close(lse.double().cpu(), lse_ref, rtol=2e-3, atol=2e-3)
  assert o.shape == (sum(lq), D)
  _close(o, ref.detach(), 2e-2)
  _close(dq, qf.grad, 3e-2)
  _close(dk, kf.grad, 3e-2)
  _close(dv, vf.grad, 3e-2)
  # the columns next to the gradient slices were not written
  assert bool((gq[:, :D] == 7.0).all()) and bool((gq[:, 2 * D:] == 7.0).all())
  assert bool((gk[:, D:2 * D] == 7.0).all())


@pytest.mark.parametrize("causal,cross", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_fwd_long_head_dims(cuda, dh, causal, cross):
  """Multi-tile forward (sequences > 64 tokens, inference): lengths up to 150, on both sides of the 64 and
  128 tile edges."""
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(11 + causal + 2 * cross + dh)
  D = H * dh
  lq = [150, 17, 65, 128, 1]
  lk = [70, 140, 9, 64, 129] if cross else lq
  (q, k, v), (qf, kf, vf) = _inputs(g, lq, lk, D, cross, cuda)
  scale = dh ** -0.5
  o, lse = capi.attention_fwd(q, k, v, _cu(lq, cuda), _cu(lk, cuda), H, max(max(lq), max(lk)), causal, scale,
                              dh=dh)
  torch.cuda.synchronize()
  ref, lse_ref = _oracle(qf, kf, vf, lq, lk, dh, scale, causal)
  torch.testing.assert_close(o.double().cpu(), ref, atol=2e-2, rtol=2e-2)
  torch.testing.assert_close(lse.double().cpu(), lse_ref, atol=2e-3, rtol=1e-3)


@pytest.mark.parametrize("dh", [24, 256])
def test_attention_unsupported_head_dim_raises(cuda, dh):
  """The C entry points answer OS2S_ERR_UNSUPPORTED, the Python layer NotImplementedError naming the set."""
  from ctypes import c_void_p
  from openseq2seq_amd import _lib, capi
  from openseq2seq_amd.parts.transformer.layers import MultiHeadAttention
  D, L = H * dh, 9
  q = torch.zeros(L, D, dtype=torch.bfloat16, device=cuda)
  cu = _cu([L], cuda)
  with pytest.raises(NotImplementedError, match="8, 16, 32, 64, 128"):
    capi.attention_fwd(q, q, q, cu, cu, H, 64, False, 1.0, dh=dh)
  with pytest.raises(NotImplementedError, match="8, 16, 32, 64, 128"):
    capi.attention_bwd(q, q, q, q, None, q, q, q, cu, cu, H, 64, False, 1.0, dh=dh)
  with pytest.raises(NotImplementedError, match="8, 16, 32, 64, 128"):
    MultiHeadAttention(None, "att", D, H, True)
  o = torch.empty_like(q)
  lse = torch.empty(L, H, dtype=torch.float32, device=cuda)
  p = lambda t: c_void_p(t.data_ptr())
  with pytest.raises(_lib.Os2sError, match="unsupported configuration"):
    _lib.C.os2s_attention_fwd(None, p(q), p(q), p(q), p(o), p(lse), p(cu), p(cu), 1, H, dh, 64, D, D, D, D, 0,
                              1.0, 1.0, 0)
  with pytest.raises(_lib.Os2sError, match="unsupported configuration"):
    _lib.C.os2s_attention_bwd(None, p(q), p(q), p(q), p(q), p(lse), p(o), p(o), p(o), p(cu), p(cu), 1, H, dh, 64,
                              D, D, D, D, D, D, D, 0, 1.0, 1.0, 0)


@pytest.mark.parametrize("dh", [32, 64])
def test_attention_invalid_stride_and_keep_prob_raise(cuda, dh):
  """The three entry points apply one set of checks whatever the head dim: a row stride shorter than a head
  (os2s_attention_fwd with ldq = 8) and keep_prob = 0 into the backwards, which divide by it, answer
  OS2S_ERR_INVALID_ARG before any launch: the output buffers keep their sentinel."""
  from ctypes import c_void_p
  from openseq2seq_amd import _lib
  D, L = H * dh, 9
  g = torch.Generator().manual_seed(3 + dh)
  q, k, v, do = (torch.randn(L, D, generator=g).to(torch.bfloat16).to(cuda) for _ in range(4))
  cu = _cu([L], cuda)
  o, dq, dk, dv = (torch.full((L, D), 7.0, dtype=torch.bfloat16, device=cuda) for _ in range(4))
  lse = torch.full((L, H), 7.0, dtype=torch.float32, device=cuda)
  delta = torch.full((L, H), 7.0, dtype=torch.float32, device=cuda)
  p = lambda t: c_void_p(t.data_ptr())
  with pytest.raises(_lib.Os2sError, match="invalid argument"):
    _lib.C.os2s_attention_fwd(None, p(q), p(k), p(v), p(o), p(lse), p(cu), p(cu), 1, H, dh, 64, 8, D, D, D, 0,
                              dh ** -0.5, 1.0, 0)
  with pytest.raises(_lib.Os2sError, match="invalid argument"):
    _lib.C.os2s_attention_bwd(None, p(q), p(k), p(v), p(do), p(lse), p(dq), p(dk), p(dv), p(cu), p(cu), 1, H, dh, 64,
                              D, D, D, D, D, D, D, 0, dh ** -0.5, 0.0, 0)
  with pytest.raises(_lib.Os2sError, match="invalid argument"):
    _lib.C.os2s_attention_bwd_long(None, p(q), p(k), p(v), p(do), p(lse), p(delta), p(dq), p(dk), p(dv), p(cu),
                                   p(cu), 1, H, dh, 128, D, D, D, D, D, D, D, 0, dh ** -0.5, 0.0, 0)
  torch.cuda.synchronize()
  for t in (o, lse, delta, dq, dk, dv):
    assert bool((t == 7.0).all())
