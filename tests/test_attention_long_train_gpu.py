"""Attention TRAINING on sequences longer than one 64-token tile (attn_fwd_long_kernel<DH, true> of csrc/attention.hip,
the multi-tile forward with dropout, and attn_bwd_long_dq_kernel / attn_bwd_long_dkv_kernel of csrc/attention_long.hpp,
the two-launch multi-tile backward) against a float64 oracle, at every head dim.

Laid out like tests/test_attention_head_dims_gpu.py, with that file's bounds — o 2e-2 of the tensor rms, gradients
3e-2, lse 2e-3: H = 3 heads, B = 5 sentences, q / k / v column slices of one [N, 3*H*dh] tensor, gradients into
column slices of buffers pre-filled with 7.0 whose neighbouring columns must stay 7.0, outputs in torch.empty
buffers. The two length sets sit on both sides of the 64, 128 and 192 tile edges and pair a sentence of 1 token
with a long partner. With keep < 1 the oracle applies the device mask, element ((b*H + h)*Lp + q)*Lp + key of
os2s_dropout_mask, Lp = max_len rounded up to 64.

Measured on an MI355X over the 60 oracle cases, as the largest |got - ref| / (rms + |ref|) of a tensor (what the
3e-2 bounds): dq 9.2e-3, dk 2.3e-2, dv 2.7e-2. The kernels round P o m / keep and dS to bf16 before the gradient
products and nothing else before the outputs; a float64 model with just those roundings gives up to 2.6e-2 (dq),
2.4e-2 (dk), 1.8e-2 (dv) on inputs of this kind, so the bounds hold without room to spare, as they do for the
one-tile kernels. (A backward that took delta = rowsum(dO o O) from the forward's bf16 O did NOT meet them: 5.5e-2
on dq where a sentence has one token, and the same float64 model with O rounded gives 0.13 under the causal mask
and 0.7 for a one-token source. Hence the fp32 delta sweep of csrc/attention_long.hpp.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HEAD_DIMS = [8, 16, 32, 64, 128]
B, H = 5, 3
LENS = [([150, 17, 65, 128, 1], [70, 140, 9, 64, 129]),
        ([64, 192, 2, 127, 66], [193, 1, 64, 65, 130])]


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


def _err(got, ref):
  """The smallest tol with which _close(got, ref, tol) passes."""
  scale = float(ref.pow(2).mean().sqrt()) + 1e-8
  return float(((got.double().cpu() - ref).abs() / (scale + ref.abs())).max())


def _fwd_bwd(capi, q, k, v, do, cq, ck, nq, nk, D, max_len, causal, scale, keep, seed, dh):
  """One forward + backward the way the layer calls them: (o, lse, dq, dk, dv, gq, gk); the gradients are column
  slices of the 7.0-filled gq / gk."""
  o, lse = capi.attention_fwd(q, k, v, cq, ck, H, max_len, causal, scale, keep, seed, dh=dh)
  gq = torch.full((nq, 3 * D), 7.0, dtype=torch.bfloat16, device=q.device)
  gk = torch.full((nk, 3 * D), 7.0, dtype=torch.bfloat16, device=q.device)
  dq, dk, dv = gq[:, D:2 * D], gk[:, :D], gk[:, 2 * D:]
  capi.attention_bwd(q, k, v, do, lse, dq, dk, dv, cq, ck, H, max_len, causal, scale, keep, seed, dh=dh)
  return o, lse, dq, dk, dv, gq, gk


@pytest.mark.parametrize("causal,cross", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("keep", [1.0, 0.9])
@pytest.mark.parametrize("lens", LENS)
@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_long_fwd_bwd(cuda, dh, lens, keep, causal, cross):
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(7 + causal + 2 * cross + dh)
  D = H * dh
  lq = lens[0]
  lk = lens[1] if cross else lq
  max_len = max(lq + lk)
  Lp = (max_len + 63) // 64 * 64
  (q, k, v), (qf, kf, vf) = _inputs(g, lq, lk, D, cross, cuda)
  do = torch.randn(sum(lq), D, generator=g).to(torch.bfloat16)
  scale = dh ** -0.5
  cq, ck = _cu(lq, cuda), _cu(lk, cuda)
  seed = 99
  o, lse, dq, dk, dv, gq, gk = _fwd_bwd(capi, q, k, v, do.to(cuda), cq, ck, sum(lq), sum(lk), D, max_len, causal,
                                        scale, keep, seed, dh)
  torch.cuda.synchronize()
  mask = None
  if keep < 1.0:      # the device mask: element ((b*H+h)*Lp + q)*Lp + key, whatever the head dim
    mask = capi.dropout_mask(seed, B * H * Lp * Lp, keep, cuda).cpu().view(B, H, Lp, Lp)
  qf, kf, vf = (t.requires_grad_(True) for t in (qf, kf, vf))
  ref, lse_ref = _oracle(qf, kf, vf, lq, lk, dh, scale, causal, mask, keep)
  ref.backward(do.double())
  torch.testing.assert_close(lse.double().cpu(), lse_ref, rtol=2e-3, atol=2e-3)
  assert o.shape == (sum(lq), D)
  _close(o, ref.detach(), 2e-2)
  for name, got, want in zip(("dq", "dk", "dv"), (dq, dk, dv), (qf.grad, kf.grad, vf.grad)):
    print("%s: error %.3e of (rms + |ref|)" % (name, _err(got, want)))
    _close(got, want, 3e-2)
  # the columns next to the gradient slices were not written
  assert bool((gq[:, :D] == 7.0).all()) and bool((gq[:, 2 * D:] == 7.0).all())
  assert bool((gk[:, D:2 * D] == 7.0).all())


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("causal,cross", [(True, False), (False, True)])
@pytest.mark.parametrize("dh", [32, 64, 128])
def test_attention_long_is_bitwise_reproducible(cuda, dh, causal, cross, deterministic):
  """Two forward + backward calls on the same inputs give the same bits, whatever the library's deterministic mode:
  every output element has one owner that sums its tiles in a fixed order (no float atomics)."""
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(3 + dh)
  D = H * dh
  lq, lk = LENS[0][0], (LENS[0][1] if cross else LENS[0][0])
  (q, k, v), _ = _inputs(g, lq, lk, D, cross, cuda)
  do = torch.randn(sum(lq), D, generator=g).to(torch.bfloat16).to(cuda)
  cq, ck = _cu(lq, cuda), _cu(lk, cuda)
  was = capi.deterministic()
  capi.set_deterministic(deterministic)
  try:
    runs = [_fwd_bwd(capi, q, k, v, do, cq, ck, sum(lq), sum(lk), D, max(lq + lk), causal, dh ** -0.5, 0.9, 5, dh)
            for _ in range(2)]
    torch.cuda.synchronize()
  finally:
    capi.set_deterministic(was)
  for a, b, name in zip(runs[0], runs[1], ("o", "lse", "dq", "dk", "dv", "gq", "gk")):
    assert torch.equal(a, b), name


@pytest.mark.parametrize("causal,cross", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_attention_long_agrees_with_one_tile_kernels(cuda, dh, causal, cross):
  """Sentences of at most 64 tokens, keep = 1: max_len = 64 launches the one-tile kernels, max_len = 128 the
  tile-walking ones. Different kernels, different summation orders: they agree within the bounds both are held
  to against the oracle, not bitwise."""
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(17 + dh)
  D = H * dh
  lq = [64, 17, 1, 33, 56]
  lk = [40, 64, 9, 2, 56] if cross else lq
  (q, k, v), _ = _inputs(g, lq, lk, D, cross, cuda)
  do = torch.randn(sum(lq), D, generator=g).to(torch.bfloat16).to(cuda)
  cq, ck = _cu(lq, cuda), _cu(lk, cuda)
  short = _fwd_bwd(capi, q, k, v, do, cq, ck, sum(lq), sum(lk), D, 64, causal, dh ** -0.5, 1.0, 0, dh)
  long_ = _fwd_bwd(capi, q, k, v, do, cq, ck, sum(lq), sum(lk), D, 128, causal, dh ** -0.5, 1.0, 0, dh)
  torch.cuda.synchronize()
  o_s, lse_s, dq_s, dk_s, dv_s = (t.double().cpu() for t in short[:5])
  o_l, lse_l, dq_l, dk_l, dv_l = long_[:5]
  torch.testing.assert_close(lse_l.double().cpu(), lse_s, rtol=2e-3, atol=2e-3)
  _close(o_l, o_s, 2e-2)
  _close(dq_l, dq_s, 3e-2)
  _close(dk_l, dk_s, 3e-2)
  _close(dv_l, dv_s, 3e-2)
