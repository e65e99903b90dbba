"""Fused MXFP8 separable convolution (csrc/sepconv1d_mx.hip): the kernel against an fp64 model (depthwise -> bf16 ->
format rule -> pointwise -> affine / ReLU / mask) within the worst-case fp32 summation bound, the refusals of the C
ABI, and the 'mxfp8_inference' switch of SepConvBN / TDNNEncoder against the bf16 chain.

The quantiser is discontinuous, so the inputs make the fp32 depthwise sum exact in any order: x is an integer of
magnitude <= 4 times a power of two per (sample, channel block) times 2^(row mod 4), the taps are integers in
[-2, 2]; every partial sum is an integer below 96 * 8 * 8 < 2^13 times the block's power of two."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# relative L2 distance of the toy separable encoder's MXFP8 output to its bf16 output: 3 x the value measured on an
# MI355X (profiles/mxfp8_sepconv_first_measurements.md); a broken layer shows as O(1)
ENCODER_REL_L2_MEASURED = 0.006387
ENCODER_REL_L2_BOUND = 3 * ENCODER_REL_L2_MEASURED


def _mx_ref(x):
  """The format rule on the CPU (as in test_conv1d_mx_gpu.py). x: bf16 [rows, K] -> (e4m3 bytes [rows, K], the scale
  bytes in the device layout [ceil(K/128), rows, 4], the dequantised values in fp64). e = floor(log2(amax)) - 8,
  byte = clamp(e + 127, 0, 254), element = RNE(clamp(x 2^-e, +-448)); an all-zero block: byte 0."""
  rows, K = x.shape
  xb = x.double().view(rows, K // 32, 32)
  amax = xb.abs().amax(-1)
  _, ex = torch.frexp(amax)
  byte = torch.where(amax > 0, (ex - 1 - 8 + 127).clamp(0, 254), torch.zeros_like(ex)).to(torch.int32)
  q = torch.ldexp(xb, (127 - byte)[..., None]).clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn)
  deq = torch.ldexp(q.double(), (byte - 127)[..., None]).view(rows, K)
  KT = (K + 127) // 128
  sc = torch.zeros((rows, KT * 4), dtype=torch.uint8)
  sc[:, :K // 32] = byte.to(torch.uint8)
  return q.view(torch.uint8).view(rows, K), sc.view(rows, KT, 4).permute(1, 0, 2).contiguous(), deq


def _weights(Cout, Cin, g):
  """bf16 [Cout, Cin]: every (row, 32-block) has its own power-of-two magnitude, so a scale routed from the wrong
  row or block moves an output by 2x or more."""
  mag = torch.exp2(((torch.arange(Cout)[:, None] + 3 * torch.arange(Cin // 32)[None, :] + 5) % 13 - 6).float())
  sign = torch.where(torch.rand((Cout, Cin), generator=g) < 0.5, -1.0, 1.0)
  return (mag.repeat_interleave(32, dim=1) * (1.0 + torch.rand((Cout, Cin), generator=g)) * sign).to(torch.bfloat16)


def _exact_inputs(B, T, Cin, K, g):
  """(x bf16 [B, T, Cin], taps fp32 [K, Cin]) of the module docstring."""
  e = (3 * torch.arange(Cin // 32)[None, None, :] + 5 * torch.arange(B)[:, None, None]) % 13 - 6 + \
      torch.arange(T)[None, :, None] % 4
  x = torch.randint(-4, 5, (B, T, Cin), generator=g).float() * torch.exp2(e.float()).repeat_interleave(32, dim=2)
  return x.to(torch.bfloat16), torch.randint(-2, 3, (K, Cin), generator=g).float()


def _model(x, d, w_deq, pad_left, in_len, cs=None, cb=None, act=0, out_len=None, f32=False):
  """(fp64 reference, elementwise bound): depthwise in fp64 (rows outside [0, in_len) zero) -> bf16 -> format rule ->
  product with the dequantised weights -> affine / ReLU / mask. Bound: Cin 2^-22 (|zq| . |w|) |ch_scale| — worst-case
  fp32 summation with one bit for a truncating accumulator — plus 2^-8 |ref| for a bf16 result."""
  B, T, Cin = x.shape
  K = d.shape[0]
  xd = x.double().clone()
  for b, n in enumerate(in_len if in_len is not None else []):
    xd[b, n:] = 0.0
  xp = torch.nn.functional.pad(xd, (0, 0, pad_left, K - 1 - pad_left))
  z = sum(xp[:, k:k + T] * d[k].double() for k in range(K)).float().to(torch.bfloat16)
  z_deq = _mx_ref(z.view(B * T, Cin))[2].view(B, T, Cin)
  ref, mag = z_deq @ w_deq.t(), z_deq.abs() @ w_deq.abs().t()
  if cs is not None:
    ref, mag = ref * cs.double() + cb.double(), mag * cs.double().abs()
  if act == 1:
    ref = ref.clamp_min(0.0)
  for b, n in enumerate(out_len if out_len is not None else []):
    ref[b, n:] = 0.0
  bound = Cin * 2.0 ** -22 * mag
  return ref, bound if f32 else bound + 2.0 ** -8 * ref.abs()


def _check(out, ref, bound):
  err = (out.double().cpu() - ref).abs()
  print("max err / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
  assert bool((err <= bound).all())


@pytest.mark.parametrize("B,Tin,Cin,Cout,K,lens,epi", [
    (1, 5, 64, 8, 1, None, "none"),                    # one tap, half channel tile, rows next to both paddings
    (2, 140, 192, 264, 33, [140, 17], "affine_relu"),  # 2nd row tile, 128 + 64 channels, 2nd column chunk + tail, ragged
    (1, 33, 64, 8, 96, None, "f32"),                   # largest window, Tin below the halo
    (2, 130, 512, 40, 3, [130, 3], "relu"),            # largest zq tile; sample ends in the halo; a tile past the length
    (3, 7, 256, 8, 2, [7, 1, 4], "affine_relu")])      # even K (SAME pads on the right), two full channel tiles
def test_kernel_against_fp64(cuda, B, Tin, Cin, Cout, K, lens, epi):
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
                              act=act, out_f32=f32)
  assert out.dtype == (torch.float32 if f32 else torch.bfloat16) and tuple(out.shape) == (B, Tin, Cout)
  _, pad_left = capi.same_padding(Tin, K, 1, 1)
  _check(out, *_model(x, d, w_deq, pad_left, lens, cs if affine else None, cb if affine else None, act, lens, f32))
  for b, n in enumerate(lens or []):
    assert not bool(out[b, n:].any())                   # rows at or past out_len: exactly zero


def test_refusals(cuda):
  from openseq2seq_amd import _lib
  f = _lib.lib().os2s_sepconv1d_fwd_mx                  # the library's own attribute: returns the status
  p = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda).data_ptr()

  def call(x=p, Cin=64, Cout=8, K=3, act=0):
    return f(None, x, p, p, p, p, None, None, None, None, 1, 16, Cin, Cout, K, 1, 1, 1, 16, 16 * Cout, Cout, 0, act)
  assert call() == 0
  for bad in (dict(Cin=576), dict(Cin=72), dict(Cin=32), dict(Cout=12), dict(K=97), dict(act=2)):
    assert call(**bad) == -3                            # OS2S_ERR_UNSUPPORTED
  assert call(x=None) == -1                             # OS2S_ERR_INVALID_ARG
  torch.cuda.synchronize()


def test_layer_switch(cuda):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.parts.cnns.conv_blocks import SepConvBN, conv_bn_actv
  from openseq2seq_amd.parts.tape import Act, Tape
  torch.manual_seed(3)
  g = torch.Generator().manual_seed(4)
  store = FlatParams(cuda)
  layer, twin = SepConvBN(store, "c", "c/bn", 64, 128, 11), SepConvBN(store, "s", "s/bn", 64, 128, 11, stride=2)
  tap1 = SepConvBN(store, "o", "o/bn", 64, 128, 1)      # one tap: folded into a 1x1 convolution
  store.finalize()
  lens_h = [50, 21, 7]
  xh, taps = _exact_inputs(3, 50, 64, 11, g)
  for L in (layer, twin, tap1):
    L.depthwise.master.copy_(taps[:L.k])
    L.gamma.master.copy_(0.5 + torch.rand(128))
    L.beta.master.copy_(torch.randn(128) * 0.2)
    L.moving_mean.copy_(torch.randn(128) * 0.1)
    L.moving_var.copy_(0.5 + torch.rand(128))
  lens = torch.tensor(lens_h, dtype=torch.int32, device=cuda)
  for b, n in enumerate(lens_h):
    xh[b, n:] = 0
  x = Act(xh.to(cuda), lens, requires_grad=False)
  lens2 = (lens + 1) // 2

  def run(L, training=False, tape=None):
    return conv_bn_actv(L, x, lens2 if L is twin else lens, "relu", training, tape).data

  def model():                                          # moving-statistics affine -> ReLU -> mask behind the fp64 chain
    w_deq = _mx_ref(layer.kernel.w16.cpu().view(128, 64))[2]
    cs = layer.gamma.master.cpu().double() / (layer.moving_var.cpu().double() + layer.eps).sqrt()
    cb = layer.beta.master.cpu().double() - layer.moving_mean.cpu().double() * cs
    return _model(xh, taps, w_deq, 5, lens_h, cs, cb, 1, lens_h)
  off = [run(layer), run(layer, tape=Tape()), run(twin), run(tap1)]
  layer.mxfp8 = twin.mxfp8 = tap1.mxfp8 = True
  y = run(layer)
  _check(y, *model())
  assert not torch.equal(y, off[0])                     # it is the other path
  # the block-end branch (identity epilogue, tiles past the lengths skipped), which the by-shape rule leaves unused
  w_deq = _mx_ref(layer.kernel.w16.cpu().view(128, 64))[2]
  _check(layer.conv_bn_stats(x, False, mx=True, out_len=lens)["y"], *_model(xh, taps, w_deq, 5, lens_h, out_len=lens_h))
  on = [run(layer, tape=Tape()), run(twin), run(tap1)]
  assert all(torch.equal(a, b) for a, b in zip(on, off[1:]))
  # the weight copy follows the store's version counter
  layer.kernel.master.mul_(2.0)
  store.refresh_compute_copies()
  _check(run(layer), *model())
  # training (batch statistics; last, it moves the moving statistics) keeps the bf16 chain
  layer.mxfp8 = False
  train_bf16 = run(layer, training=True)
  layer.mxfp8 = True
  assert torch.equal(run(layer, training=True), train_bf16)


def test_encoder_switch(cuda):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.tdnn_encoder import TDNNEncoder
  # two residual separable blocks in the manner of QuartzNet, plain ReLU (a clipped ReLU keeps every layer on bf16);
  # the first layer of each block takes the fused kernel, the block ends keep bf16 by the measured rule
  sep = lambda c: dict(type="sep_conv1d", repeat=2, kernel_size=[7], stride=[1], num_channels=c, padding="SAME",
                       dilation=[1], residual=True)
  layers = [sep(128), sep(256)]

  def run(**extra):
    torch.manual_seed(0)
    store = FlatParams(cuda)
    enc = TDNNEncoder(dict({"convnet_layers": layers, "dropout_keep_prob": 1.0, "activation_fn": "relu",
                            "use_conv_mask": True, "dtype": "mixed"}, **extra), None, mode="eval").build(store, 64)
    store.finalize()
    g = torch.Generator().manual_seed(5)
    x = torch.randn((4, 300, 64), generator=g).to(torch.bfloat16).to(cuda)
    lens = torch.tensor([300, 257, 120, 9], dtype=torch.int32, device=cuda)
    return enc.encode({"source_tensors": [x, lens]})["outputs"]
  off, on = run().float(), run(mxfp8_inference=True).float()      # the bf16 chain is the parent's behaviour
  assert bool(torch.isfinite(on).all())
  rel = float((on - off).norm() / off.norm())
  print("encoder rel L2 (mxfp8 vs bf16) = %.4g" % rel)
  assert 0.0 < rel < ENCODER_REL_L2_BOUND
