"""Kernel-level tests of csrc/conv2d_toeplitz.hip and of its user encoders/ds2_encoder.py:Conv2dBN, beyond the
odd-KF, stride-2 SAME layers the whole-model tests run: VALID padding, an even KF, stride 1 in frequency, an odd
Fi, the asymmetric SAME pad (padF = 0, pad on the right only) and KF > Fi.
  * toeplitz_expand_kernel is a pure gather: bit for bit against toeplitz_expand_ref, +0 outside the band.
  * toeplitz_reduce_kernel ACCUMULATES into dw: pre-filled, got - prefill against the float64 adjoint.
  * the expansion fed to the real conv1d forward / weight-gradient kernels against oracle.ds2.conv2d_tf (float64),
    with the tolerances of test_conv1d_gpu.py.
  * Conv2dBN forward and backward on a Tape against conv2d_tf + batch_norm_train + relu, per element, with the
    tolerances of test_batchnorm_gpu.py (no cosine bounds).
The references are tied to the TF-semantics oracle on the CPU in tests/test_oracle_gst.py."""
import pytest
import torch

import _gst_ref as R
from oracle import cnn as ocnn, ds2 as ods

pytestmark = pytest.mark.gpu

F64 = torch.float64
CASES = R.TOEPLITZ_CASES
B, T = 2, 13


def _geometry(capi, Fi, KF, sF, padding):
  """(Fo, padF) as Conv2dBN.__init__ derives them."""
  if padding == "SAME":
    Fo, padF = capi.same_padding(Fi, KF, sF, 1)
  else:
    Fo, padF = (Fi - KF) // sF + 1, 0
  assert (Fo, padF) == R.toeplitz_geometry(Fi, KF, sF, padding)
  return Fo, padF


def _time_geometry(capi, KT, sT, padding):
  return capi.same_padding(T, KT, sT, 1) if padding == "SAME" else capi.valid_padding(T, KT, sT, 1)


def _bits16(t):
  return t.detach().cpu().view(torch.int16)


@pytest.mark.parametrize("KT,KF,Cin,Cout,Fi,sF,padding", CASES)
def test_expand_is_bit_exact(cuda, KT, KF, Cin, Cout, Fi, sF, padding):
  from openseq2seq_amd import capi
  Fo, padF = _geometry(capi, Fi, KF, sF, padding)
  g = torch.Generator().manual_seed(KT * 100 + KF + Fi)
  w = torch.randn(KT, KF, Cin, Cout, generator=g)
  w[w == 0] = 1.0                                                        # the band is where W' != 0
  out = torch.full((KT, Fo * Cout, Fi * Cin), -7.0, dtype=torch.bfloat16, device=cuda)   # sentinel
  capi.conv2d_toeplitz_expand(w.to(cuda), Fi, Fo, sF, padF, out)
  torch.cuda.synchronize()
  want = R.toeplitz_expand_ref(w, Fi, Fo, sF, padF).to(torch.bfloat16)
  assert torch.equal(_bits16(out), _bits16(want))
  band = R.toeplitz_expand_ref(torch.ones_like(w), Fi, Fo, sF, padF) != 0
  assert 0 < int(band.sum()) < band.numel()
  assert not _bits16(out)[~band].any()                                    # exactly +0 outside the band
  assert bool((out.cpu()[band] != 0).all())


@pytest.mark.parametrize("KT,KF,Cin,Cout,Fi,sF,padding", CASES)
def test_reduce_accumulates_the_adjoint(cuda, KT, KF, Cin, Cout, Fi, sF, padding):
  """Each element sums at most Fo <= 16 fp32 terms in a fixed order, then one add onto the prefill: the bound is
  derived, |err| <= 2**-20 * max|ref| + 2**-22 * max|prefill|."""
  from openseq2seq_amd import capi
  Fo, padF = _geometry(capi, Fi, KF, sF, padding)
  assert Fo <= 16
  g = torch.Generator().manual_seed(KT * 10 + KF + 7 * Fi)
  dwexp = torch.randn(KT, Fo * Cout, Fi * Cin, generator=g)
  pre = torch.randn(KT, KF, Cin, Cout, generator=g)
  dw = pre.clone().to(cuda)
  capi.conv2d_toeplitz_reduce(dwexp.to(cuda), Fi, Fo, sF, padF, dw)
  torch.cuda.synchronize()
  ref = R.toeplitz_reduce_ref(dwexp.to(F64), KF, Cin, Cout, Fi, Fo, sF, padF)
  got = dw.cpu().to(F64) - pre.to(F64)
  err = float((got - ref).abs().max())
  bound = 2.0 ** -20 * float(ref.abs().max()) + 2.0 ** -22 * float(pre.abs().max())
  print("reduce err %.3e bound %.3e" % (err, bound))
  assert float(ref.abs().max()) > 0 and err <= bound, (err, bound)


def _conv_inputs(KT, KF, Cin, Cout, Fi, seed):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(B, T, Fi * Cin, generator=g).to(torch.bfloat16)
  w = torch.randn(KT, KF, Cin, Cout, generator=g) * (KT * min(KF, Fi) * Cin) ** -0.5
  return g, x, w


@pytest.mark.parametrize("sT", [1, 2])
@pytest.mark.parametrize("KT,KF,Cin,Cout,Fi,sF,padding", CASES)
def test_expansion_through_conv1d_fwd_and_wgrad(cuda, KT, KF, Cin, Cout, Fi, sF, padding, sT):
  from openseq2seq_amd import capi
  Fo, padF = _geometry(capi, Fi, KF, sF, padding)
  tout, pl = _time_geometry(capi, KT, sT, padding)
  g, x, w = _conv_inputs(KT, KF, Cin, Cout, Fi, KT * 1000 + KF * 10 + Fi + sT)
  wexp = torch.empty((KT, Fo * Cout, Fi * Cin), dtype=torch.bfloat16, device=cuda)
  capi.conv2d_toeplitz_expand(w.to(cuda), Fi, Fo, sF, padF, wexp)
  xd = x.to(cuda)
  y = capi.conv1d_fwd(xd, wexp, stride=sT, pad_left=pl, tout=tout)
  # ---- float64 conv2d on the bf16-rounded input and kernel
  w64 = w.to(torch.bfloat16).to(F64).requires_grad_(True)
  ref = ods.conv2d_tf(x.to(F64).view(B, T, Fi, Cin), w64, [sT, sF], padding)
  assert tuple(ref.shape) == (B, tout, Fo, Cout)
  dy = torch.randn(B, tout, Fo * Cout, generator=g).to(torch.bfloat16)
  (dw_ref,) = torch.autograd.grad(ref, w64, dy.to(F64).view(B, tout, Fo, Cout))
  ref = ref.detach().reshape(B, tout, Fo * Cout)
  torch.cuda.synchronize()
  assert tuple(y.shape) == tuple(ref.shape)
  rms = float(ref.pow(2).mean().sqrt())
  torch.testing.assert_close(y.cpu().to(F64), ref, rtol=1e-2, atol=1e-2 * rms)
  # ---- weight gradient: conv1d_wgrad, folded back onto the master kernel
  dwexp = capi.conv1d_wgrad(xd, dy.to(cuda), KT, stride=sT, pad_left=pl)
  dw = torch.zeros(KT, KF, Cin, Cout, device=cuda)
  capi.conv2d_toeplitz_reduce(dwexp, Fi, Fo, sF, padF, dw)
  torch.cuda.synchronize()
  rms = float(dw_ref.pow(2).mean().sqrt())
  torch.testing.assert_close(dw.cpu().to(F64), dw_ref, rtol=2e-3, atol=2e-3 * rms)


LAYER_CASES = [c for c in CASES if c[6] == "VALID" or c[1] % 2 == 0 or c == (3, 3, 8, 8, 7, 2, "SAME")]
assert len(LAYER_CASES) == 3


@pytest.mark.parametrize("KT,KF,Cin,Cout,Fi,sF,padding", LAYER_CASES)
def test_conv2dbn_layer_fwd_bwd(cuda, KT, KF, Cin, Cout, Fi, sF, padding):
  """sT = 2 on an odd Tin = 13: the zero-stuffed (transposed-convolution) data-gradient path."""
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.ds2_encoder import Conv2dBN
  from openseq2seq_amd.parts.tape import Act, Tape
  sT, eps = 2, 1e-3
  torch.manual_seed(KT + KF)
  store = FlatParams(cuda)
  layer = Conv2dBN(store, "conv", Fi, Cin, Cout, [KT, KF], [sT, sF], padding, 0.9, eps, 0.0)
  store.finalize()
  g = torch.Generator().manual_seed(KT * 100 + KF * 10 + Fi)
  layer.gamma.master.add_((torch.rand(Cout, generator=g) - 0.5).to(cuda))
  layer.beta.master.add_((torch.randn(Cout, generator=g) * 0.3).to(cuda))
  store.refresh_compute_copies()
  x = torch.randn(B, T, Fi * Cin, generator=g).to(torch.bfloat16)
  xa = Act(x.to(cuda), None, requires_grad=True)
  tape = Tape()
  store.zero_grads()
  out = layer.forward(xa, "relu", True, tape)
  tout = out.data.shape[1]
  dout = torch.randn(B, tout, layer.Fo * Cout, generator=g).to(torch.bfloat16)
  out.grad = dout.to(cuda)
  tape.backward()
  torch.cuda.synchronize()
  # ---- reference: conv2d_tf + batch_norm_train + relu on the bf16-rounded kernel
  w = layer.kernel.master.cpu().to(torch.bfloat16).float().requires_grad_(True)
  gm = layer.gamma.master.cpu().clone().requires_grad_(True)
  bt = layer.beta.master.cpu().clone().requires_grad_(True)
  xr = x.float().requires_grad_(True)
  y = ods.conv2d_tf(xr.view(B, T, Fi, Cin), w, [sT, sF], padding)
  Bq, Tq, Fq, Cq = y.shape
  assert (Tq, Fq, Cq) == (tout, layer.Fo, Cout)
  yn = ocnn.batch_norm_train(y.reshape(Bq, Tq * Fq, Cq), gm, bt, eps)[0]
  ref = torch.relu(yn).reshape(Bq, Tq, Fq * Cq)
  (ref * dout.float()).sum().backward()

  def check(name, got, want):
    got, want = got.detach().float().cpu().reshape(want.shape), want.detach()
    rms = float(want.pow(2).mean().sqrt())
    print("layer %-12s max err %.3e rms(ref) %.3e" % (name, float((got - want).abs().max()), rms))
    assert rms > 0, name
    torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-2 * rms, msg=lambda m: name + ": " + m)
  check("out", out.data, ref)
  check("x.grad", xa.grad, xr.grad)
  check("kernel.grad", layer.kernel.grad, w.grad)
  check("gamma.grad", layer.gamma.grad, gm.grad)
  check("beta.grad", layer.beta.grad, bt.grad)
