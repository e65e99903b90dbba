"""OS2S_LAUNCH_LDS (csrc/os2s_common.hpp) opts a kernel into more than 64 KB of dynamic LDS per (launch site,
device). Two ways a latch keyed on the wrong thing shows:

 * second device: an entry point that has run on device 0 runs on device 1 from the same host inputs; both
   results meet the oracle and tolerance of that entry point's own test and equal each other bit for bit (no
   atomics at these settings: one owner per output element);
 * repeat and interleave: two template instances of one launch site, alternately, on device 0; every call
   returns the bits of its own first call.

Shapes are the smallest that reach the opt-in; the bytes are those of the host code next to each launch."""
import pytest
import torch

import test_attention_head_dims_gpu as ahd

pytestmark = pytest.mark.gpu

from oracle import cnn  # noqa: E402

DH, HEADS, LENS = 128, 2, [64, 37]


def _bits(t):
  return t.detach().cpu().contiguous().view(torch.uint8)


def _same_bits(a, b):
  return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _on(dev, fn):
  with torch.cuda.device(dev):
    out = fn(dev)
    torch.cuda.synchronize(dev)
  return tuple(t.cpu() for t in out)


# ---- capi.conv1d_wgrad, stride 2, K = 3: the lockstep kernel conv1d_wgrad_kernel<2, 128>. COT = 128 (Cout < 512),
# xrows = 63 * 2 + 1 + 1 = 128: smem = 2 * 64 * 2 * 128 + 2 * 128 * 256 = 98 304 bytes.
def _wgrad_case():
  B, T, C, K, s = 2, 128, 128, 3, 2
  g = torch.Generator().manual_seed(31)
  x = torch.randn(B, T, C, generator=g).to(torch.bfloat16)
  w_tf = (torch.randn(K, C, C, generator=g) * 0.05).requires_grad_(True)
  lens = torch.tensor([T, 77], dtype=torch.int32)
  y = cnn.conv1d_tf(x.float(), w_tf, s, 1, "SAME", mask_len=lens)
  dy = torch.randn(y.shape, generator=g).to(torch.bfloat16)
  y.backward(dy.float())
  ref = cnn.to_dev_layout(w_tf.grad)

  def run(dev):
    from openseq2seq_amd import capi
    return (capi.conv1d_wgrad(x.to(dev), dy.to(dev), K, stride=s, in_len=lens.to(dev), accumulate=False),)

  def check(out):      # the bound of test_conv1d_gpu.test_conv_wgrad (written out there, not a helper)
    scale = float(ref.pow(2).mean().sqrt()) + 1e-6
    torch.testing.assert_close(out[0], ref, rtol=2e-3, atol=2e-3 * scale)
  return run, check


# ---- capi.attention_fwd / attention_bwd at dh = 128, lengths <= 64: attn_fwd_kernel<128, false> with
# kFwdWaves * kImgs * 8192 = 4 * 2 * 8192 = 65 536 bytes (exactly the default limit: opted in), and
# attn_bwd_kernel<128, false> with attn_bwd_lds<128>() = 81 920 bytes.
def _attention_case():
  D = HEADS * DH
  scale = DH ** -0.5
  g = torch.Generator().manual_seed(5)
  q, k, v, do = (torch.randn(sum(LENS), D, generator=g).to(torch.bfloat16) for _ in range(4))

  def run(dev):
    from openseq2seq_amd import capi
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    cu = ahd._cu(LENS, dev)
    o, lse = capi.attention_fwd(qd, kd, vd, cu, cu, HEADS, 64, False, scale, dh=DH)
    dq, dk, dv = (torch.empty(sum(LENS), D, dtype=torch.bfloat16, device=dev) for _ in range(3))
    capi.attention_bwd(qd, kd, vd, do.to(dev), lse, dq, dk, dv, cu, cu, HEADS, 64, False, scale, dh=DH)
    return o, lse, dq, dk, dv

  # ahd._oracle splits its rows into ahd.H heads. Heads are independent, so the HEADS heads here are followed by
  # zero heads up to that count and the oracle's first HEADS heads are the reference.
  assert ahd.H >= HEADS
  pad = torch.zeros(sum(LENS), (ahd.H - HEADS) * DH, dtype=torch.float64)
  qf, kf, vf = (t.double().requires_grad_(True) for t in (q, k, v))
  ref, lse_ref = ahd._oracle(*(torch.cat([t, pad], 1) for t in (qf, kf, vf)), LENS, LENS, DH, scale, False)
  ref, lse_ref = ref[:, :D], lse_ref[:, :HEADS]
  ref.backward(do.double())

  def check(out):      # the bounds of test_attention_head_dims_gpu.test_attention_fwd_bwd_head_dims
    o, lse, dq, dk, dv = out
    torch.testing.assert_close(lse.double(), lse_ref, rtol=2e-3, atol=2e-3)
    ahd._close(o, ref.detach(), 2e-2)
    ahd._close(dq, qf.grad, 3e-2)
    ahd._close(dk, kf.grad, 3e-2)
    ahd._close(dv, vf.grad, 3e-2)
  return run, check


# ---- capi.gemm_nt (gemm_pp.hip): gemm_pp_kernel always takes its A ring of 3 + W ring of 2 =
# 5 * 256 * 128 = 163 840 bytes. M = 200 (a partial 256-row tile), N = 264 (two column tiles), K = 128: two
# units, no split (fmax = K / 64 / 8 = 0), so one owner per output element.
def _gemm_case():
  M, N, K = 200, 264, 128
  g = torch.Generator().manual_seed(17)
  a = torch.randn(M, K, generator=g).to(torch.bfloat16)
  w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
  ref = a.float() @ w.float().t()

  def run(dev):
    from openseq2seq_amd import capi
    return (capi.gemm_nt(a.to(dev), w.to(dev)),)

  def check(out):      # the bf16 bound of test_gemm_gpu.test_gemm_nt_plain (written out there, not a helper)
    scale = float(ref.pow(2).mean().sqrt())
    torch.testing.assert_close(out[0].float(), ref, rtol=1e-2, atol=1e-2 * scale)
  return run, check


CASES = (_wgrad_case, _attention_case, _gemm_case)


def test_second_device_is_opted_in_too():
  if torch.cuda.device_count() < 2:
    pytest.skip("needs a second GPU: torch.cuda.device_count() < 2")
  for case in CASES:
    run, check = case()
    out0 = _on(torch.device("cuda:0"), run)
    out1 = _on(torch.device("cuda:1"), run)
    check(out0)
    check(out1)
    assert _same_bits(out0, out1), case.__name__


def test_two_instances_of_one_site_interleaved(cuda):
  """attention_fwd at dh = 128: attn_fwd_kernel<128, false> (keep_prob = 1) and <128, true> (keep_prob < 1),
  65 536 bytes each, alternately, three times each. Before that, the cases of the second-device test run on this
  device, twice each: their inputs, oracles and bounds do not wait for a machine with two devices, and a second
  call of an opted-in site returns the bits of the first."""
  from openseq2seq_amd import capi
  for case in CASES:
    run, check = case()
    out = _on(cuda, run)
    check(out)
    assert _same_bits(out, _on(cuda, run)), case.__name__
  D = HEADS * DH
  g = torch.Generator().manual_seed(23)
  q, k, v = (torch.randn(sum(LENS), D, generator=g).to(torch.bfloat16).to(cuda) for _ in range(3))
  cu = ahd._cu(LENS, cuda)
  first = {}
  for _ in range(3):
    for keep in (1.0, 0.9):
      out = capi.attention_fwd(q, k, v, cu, cu, HEADS, 64, False, DH ** -0.5, keep, 99, dh=DH)
      torch.cuda.synchronize()
      assert bool(torch.isfinite(out[0].float()).all())
      assert _same_bits(out, first.setdefault(keep, out)), keep
  assert not _same_bits(first[1.0][:1], first[0.9][:1])      # the two instances do compute different things
