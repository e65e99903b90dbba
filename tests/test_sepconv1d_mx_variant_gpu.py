"""The matrix-pipe variant of the fused MXFP8 separable convolution (variant 1 of os2s_sepconv1d_fwd_mx_variant,
csrc/sepconv1d_mx.hip) against the fp64 model and elementwise bound of test_sepconv1d_mx_gpu.py, on inputs whose fp32
depthwise sums are exact in any order; the low halves of the hi + lo tap pair; the refusals of the new entry; and the
by-shape choice of a 512-wide SepConvBN."""
import pytest
import torch

from test_sepconv1d_mx_gpu import _check, _exact_inputs, _model, _mx_ref, _weights

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,Tin,Cin,Cout,K,lens,epi", [
    (1, 5, 64, 8, 1, None, "none"),                    # one window step, rows next to both paddings, half a channel tile
    (1, 40, 64, 8, 17, None, "none"),                  # a window of 32 positions: the last K of one MFMA window step
    (1, 40, 64, 8, 18, None, "none"),                  # 33 positions: two steps; even K (SAME pads on the right)
    (1, 33, 64, 8, 96, None, "f32"),                   # largest window, Tin below the halo
    (2, 140, 192, 264, 33, [140, 17], "affine_relu"),  # 2nd row tile, 128 + 64 channels, 2nd column chunk + tail, ragged
    (2, 130, 512, 40, 3, [130, 3], "relu")])           # largest zq; sample ends in the halo; a tile past the length
def test_variant1_against_fp64(cuda, B, Tin, Cin, Cout, K, lens, epi):
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(B + 3 * Tin + 5 * Cin + 7 * K)
  x, d = _exact_inputs(B, Tin, Cin, K, g)
  wq, ws, w_deq = _mx_ref(_weights(Cout, Cin, g))
  affine, act, f32 = epi.startswith("affine"), int(epi.endswith("relu")), epi == "f32"
  cs = (0.5 + torch.rand(Cout, generator=g)) * torch.where(torch.rand(Cout, generator=g) < 0.5, -1.0, 1.0)
  cb = torch.randn(Cout, generator=g) * 64.0
  ln = torch.tensor(lens, dtype=torch.int32, device=cuda) if lens else None
  out = capi.sepconv1d_fwd_mx(x.to(cuda), d.to(cuda), wq.to(cuda), ws.to(cuda), in_len=ln, out_len=ln,
                              ch_scale=cs.to(cuda) if affine else None, ch_shift=cb.to(cuda) if affine else None,
                              act=act, out_f32=f32, variant=1)
  assert out.dtype == (torch.float32 if f32 else torch.bfloat16) and tuple(out.shape) == (B, Tin, Cout)
  _, pad_left = capi.same_padding(Tin, K, 1, 1)
  _check(out, *_model(x, d, w_deq, pad_left, lens, cs if affine else None, cb if affine else None, act, lens, f32))
  for b, n in enumerate(lens or []):
    assert not bool(out[b, n:].any())                   # rows at or past out_len: exactly zero


def test_low_tap_halves_are_live(cuda):
  """Taps 1 + 2^-9 and -1 in turn: their bf16 roundings cancel, z is carried by the low halves alone. x is constant
  per channel (an integer times a power of two), so every sum is exact in fp32: z = (K / 2) 2^-9 x away from the
  borders."""
  from openseq2seq_amd import capi
  B, T, Cin, Cout, K = 1, 40, 64, 8, 18
  g = torch.Generator().manual_seed(11)
  x = (torch.randint(1, 5, (1, 1, Cin), generator=g).float() * torch.exp2(torch.arange(Cin).float() % 5)) \
      .expand(B, T, Cin).contiguous().to(torch.bfloat16)
  d = torch.where(torch.arange(K)[:, None] % 2 == 0, 1.0 + 2.0 ** -9, -1.0).expand(K, Cin).contiguous()
  wq, ws, w_deq = _mx_ref(_weights(Cout, Cin, g))
  out = capi.sepconv1d_fwd_mx(x.to(cuda), d.to(cuda), wq.to(cuda), ws.to(cuda), out_f32=True, variant=1)
  _, pad_left = capi.same_padding(T, K, 1, 1)
  ref, bound = _model(x, d, w_deq, pad_left, None, f32=True)
  assert bool((ref[0, T // 2].abs() > 0).all())         # the model's z is not zero
  _check(out, ref, bound)


def test_refusals_and_variant0(cuda):
  from openseq2seq_amd import _lib, capi
  f = _lib.lib().os2s_sepconv1d_fwd_mx_variant          # the library's own attribute: returns the status
  p = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda).data_ptr()

  def call(variant=1, Cin=64, Cout=8, K=3, act=0):
    return f(None, p, p, p, p, p, None, None, None, None, 1, 16, Cin, Cout, K, 1, 1, 1, 16, 16 * Cout, Cout, 0, act,
             variant)
  assert call() == 0 and call(variant=0) == 0 and call(variant=-1) == 0
  assert call(variant=2) == -1 and call(variant=-2) == -1          # OS2S_ERR_INVALID_ARG
  for bad in (dict(Cin=576), dict(Cin=72), dict(K=97), dict(Cout=12), dict(act=2)):
    assert call(**bad) == -3                                       # OS2S_ERR_UNSUPPORTED
  torch.cuda.synchronize()
  # variant 0 through the new entry is the old entry
  g = torch.Generator().manual_seed(5)
  x, d = _exact_inputs(2, 140, 192, 33, g)
  wq, ws, _ = _mx_ref(_weights(72, 192, g))
  x, d, wq, ws = x.to(cuda), d.to(cuda), wq.to(cuda), ws.to(cuda)
  new = capi.sepconv1d_fwd_mx(x, d, wq, ws, act=1, variant=0)
  old = torch.empty_like(new)
  assert _lib.lib().os2s_sepconv1d_fwd_mx(None, x.data_ptr(), d.data_ptr(), wq.data_ptr(), ws.data_ptr(),
                                          old.data_ptr(), None, None, None, None, 2, 140, 192, 72, 33, 1, 1, 16, 140,
                                          140 * 72, 72, 0, 1) == 0
  assert torch.equal(new, old)


def test_layer_switch_512(cuda):
  """A plain 512 -> 128 layer, K 11: the measured rule (conv_blocks.mx_sep_wins) takes the fused kernel with variant 1
  there in eval mode without a tape; with a tape or in training the layer keeps the bf16 chain."""
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.parts.cnns.conv_blocks import SepConvBN, conv_bn_actv, mx_sep_variant
  from openseq2seq_amd.parts.tape import Act, Tape
  torch.manual_seed(3)
  g = torch.Generator().manual_seed(4)
  store = FlatParams(cuda)
  layer = SepConvBN(store, "c", "c/bn", 512, 128, 11)
  store.finalize()
  lens_h = [50, 21, 7]
  xh, taps = _exact_inputs(3, 50, 512, 11, g)
  layer.depthwise.master.copy_(taps)
  layer.gamma.master.copy_(0.5 + torch.rand(128))
  layer.beta.master.copy_(torch.randn(128) * 0.2)
  layer.moving_mean.copy_(torch.randn(128) * 0.1)
  layer.moving_var.copy_(0.5 + torch.rand(128))
  lens = torch.tensor(lens_h, dtype=torch.int32, device=cuda)
  for b, n in enumerate(lens_h):
    xh[b, n:] = 0
  x = Act(xh.to(cuda), lens, requires_grad=False)

  def run(training=False, tape=None):
    return conv_bn_actv(layer, x, lens, "relu", training, tape).data
  off = [run(), run(tape=Tape())]
  layer.mxfp8 = True
  assert mx_sep_variant(512, 128, 11) == 1
  y = run()
  w_deq = _mx_ref(layer.kernel.w16.cpu().view(128, 512))[2]
  cs = layer.gamma.master.cpu().double() / (layer.moving_var.cpu().double() + layer.eps).sqrt()
  cb = layer.beta.master.cpu().double() - layer.moving_mean.cpu().double() * cs
  _check(y, *_model(xh, taps, w_deq, 5, lens_h, cs, cb, 1, lens_h))
  assert not torch.equal(y, off[0])                     # it is the other path
  assert torch.equal(run(tape=Tape()), off[1])
  layer.mxfp8 = False
  train_bf16 = run(training=True)                       # last: it moves the moving statistics
  layer.mxfp8 = True
  assert torch.equal(run(training=True), train_bf16)
