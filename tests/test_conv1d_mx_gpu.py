"""MXFP8 inference convolution (csrc/conv1d_mx.hip): the kernel against the fp64 convolution of the dequantised
operands within the worst-case fp32 summation bound, the refusals of the C ABI, and the 'mxfp8_inference' switch of
ConvBN / TDNNEncoder against the bf16 path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# relative L2 distance of the toy TDNN encoder's MXFP8 output to its bf16 output: 3 x the value measured on an MI355X
# (profiles/mxfp8_conv_first_measurements.md); a broken layer shows as O(1)
ENCODER_REL_L2_MEASURED = 0.06555
ENCODER_REL_L2_BOUND = 3 * ENCODER_REL_L2_MEASURED


def _mx_ref(x):
  """The format rule on the CPU. x: bf16 [rows, K] -> (e4m3 bytes [rows, K], the scale bytes in the device layout
  [ceil(K/128), rows, 4], the dequantised values in fp64). e = floor(log2(amax)) - 8, byte = clamp(e + 127, 0, 254),
  element = RNE(clamp(x 2^-e, +-448)); an all-zero block: byte 0."""
  rows, K = x.shape
  xb = x.double().view(rows, K // 32, 32)
  amax = xb.abs().amax(-1)
  _, ex = torch.frexp(amax)                         # amax = m 2^ex, m in [0.5, 1): floor(log2) = ex - 1
  byte = torch.where(amax > 0, (ex - 1 - 8 + 127).clamp(0, 254), torch.zeros_like(ex)).to(torch.int32)
  q = torch.ldexp(xb, (127 - byte)[..., None]).clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn)
  deq = torch.ldexp(q.double(), (byte - 127)[..., None]).view(rows, K)
  KT = (K + 127) // 128
  sc = torch.zeros((rows, KT * 4), dtype=torch.uint8)
  sc[:, :K // 32] = byte.to(torch.uint8)
  return q.view(torch.uint8).view(rows, K), sc.view(rows, KT, 4).permute(1, 0, 2).contiguous(), deq


def _operand(n_outer, n_inner, C, g, shift):
  """bf16 [n_outer * n_inner, C]: every (outer, inner, 32-block) has its own power-of-two magnitude — outer = sample
  / tap, inner = time / cout — so a scale routed from the wrong row, block or tap moves an output by 2x or more."""
  r = torch.arange(n_outer * n_inner)[:, None]
  blk = torch.arange(C // 32)[None, :]
  mag = torch.exp2(((r % n_inner + 3 * blk + 5 * (r // n_inner) + shift) % 13 - 6).float()).repeat_interleave(32, dim=1)
  mant = 1.0 + torch.rand((n_outer * n_inner, C), generator=g)
  sign = torch.where(torch.rand((n_outer * n_inner, C), generator=g) < 0.5, -1.0, 1.0)
  return (mag * mant * sign).to(torch.bfloat16)


def _conv_ref(x_deq, w_deq, dil, pad_left, in_len, cs=None, cb=None, act=0, out_len=None, f32=False):
  """(fp64 reference, elementwise bound) of the SAME-shaped stride-1 convolution: unfold over the taps, rows outside
  [0, in_len) zero. Bound: Cin K 2^-22 (|a| conv |w|) |ch_scale| — worst-case fp32 summation with one bit for a
  truncating accumulator — plus 2^-8 |ref| for a bf16 result."""
  B, T, Cin = x_deq.shape
  K = w_deq.shape[0]
  x = x_deq.clone()
  for b, n in enumerate(in_len if in_len is not None else []):
    x[b, n:] = 0.0
  xp = torch.nn.functional.pad(x, (0, 0, pad_left, (K - 1) * dil - pad_left))
  ref = sum(xp[:, k * dil:k * dil + T] @ w_deq[k].t() for k in range(K))
  mag = sum(xp[:, k * dil:k * dil + T].abs() @ w_deq[k].abs().t() for k in range(K))
  if cs is not None:
    ref, mag = ref * cs.double() + cb.double(), mag * cs.double().abs()
  if act == 1:
    ref = ref.clamp_min(0.0)
  for b, n in enumerate(out_len if out_len is not None else []):
    ref[b, n:] = 0.0
  bound = Cin * K * 2.0 ** -22 * mag
  return ref, bound if f32 else bound + 2.0 ** -8 * ref.abs()


def _check(out, ref, bound):
  err = (out.double().cpu() - ref).abs()
  print("max err / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
  assert bool((err <= bound).all())


@pytest.mark.parametrize("B,Tin,Cin,Cout,K,dil,lens,epi", [
    (1, 5, 64, 8, 1, 1, None, "none"),                     # one tap, half channel tile, rows next to the padding
    (2, 40, 192, 264, 3, 2, [40, 17], "affine_relu"),      # dilation, 128 + 64 channels, 2nd column tile, ragged
    (1, 300, 128, 8, 11, 1, None, "affine"),               # second row tile, slab wider than the tile
    (2, 258, 256, 40, 5, 1, [258, 3], "relu"),             # sample ends inside the halo; a tile wholly past the length
    (1, 33, 64, 264, 33, 2, None, "f32"),                  # (K-1) dil = 64: the largest slab; Tin below the halo
    (3, 7, 1024, 8, 2, 1, [7, 1, 4], "affine_relu")])      # even K (SAME pads right), eight channel tiles
def test_conv_against_fp64(cuda, B, Tin, Cin, Cout, K, dil, lens, epi):
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(B + 3 * Tin + 5 * Cin + 7 * K)
  xq, xs, x_deq = _mx_ref(_operand(B, Tin, Cin, g, 0))
  wq, ws, w_deq = _mx_ref(_operand(K, Cout, Cin, g, 5))
  affine, act, f32 = epi.startswith("affine"), int(epi.endswith("relu")), epi == "f32"
  cs = (0.5 + torch.rand(Cout, generator=g)) * torch.where(torch.rand(Cout, generator=g) < 0.5, -1.0, 1.0)
  cb = torch.randn(Cout, generator=g) * 64.0
  ln = torch.tensor(lens, dtype=torch.int32, device=cuda) if lens else None
  out = capi.conv1d_fwd_mx(xq.view(B, Tin, Cin).to(cuda), xs.to(cuda), wq.to(cuda), ws.to(cuda), k=K, dil=dil,
                           in_len=ln, out_len=ln, ch_scale=cs.to(cuda) if affine else None,
                           ch_shift=cb.to(cuda) if affine else None, act=act, out_f32=f32)
  assert out.dtype == (torch.float32 if f32 else torch.bfloat16) and tuple(out.shape) == (B, Tin, Cout)
  _, pad_left = capi.same_padding(Tin, K, 1, dil)
  _check(out, *_conv_ref(x_deq.view(B, Tin, Cin), w_deq.view(K, Cout, Cin), dil, pad_left, lens,
                         cs if affine else None, cb if affine else None, act, lens, f32))
  for b, n in enumerate(lens or []):
    assert not bool(out[b, n:].any())                   # rows at or past out_len: exactly zero


def test_refusals(cuda):
  from openseq2seq_amd import _lib
  f = _lib.lib().os2s_conv1d_fwd_mx                     # the library's own attribute: returns the status
  p = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda).data_ptr()

  def call(x=p, Cin=64, Cout=8, K=3, dil=1, act=0):
    return f(None, x, p, p, p, p, None, None, None, None, 1, 16, Cin, Cout, K, dil, 0, 16, 16 * Cout, Cout, 0, act)
  assert call() == 0
  for bad in (dict(K=66), dict(Cin=72), dict(Cin=32), dict(Cout=12), dict(act=2)):      # K = 66: (K-1) dil = 65
    assert call(**bad) == -3                            # OS2S_ERR_UNSUPPORTED
  assert call(x=None) == -1                             # OS2S_ERR_INVALID_ARG
  torch.cuda.synchronize()


def test_layer_switch(cuda):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.parts.cnns.conv_blocks import ConvBN, conv_bn_actv
  from openseq2seq_amd.parts.tape import Act, Tape
  torch.manual_seed(3)
  store = FlatParams(cuda)
  layer, twin = ConvBN(store, "c", "c/bn", 64, 128, 11), ConvBN(store, "s", "s/bn", 64, 128, 11, stride=2)
  store.finalize()
  for L in (layer, twin):
    L.gamma.master.copy_(0.5 + torch.rand(128))
    L.beta.master.copy_(torch.randn(128) * 0.2)
    L.moving_mean.copy_(torch.randn(128) * 0.1)
    L.moving_var.copy_(0.5 + torch.rand(128))
  lens_h = [50, 21, 7]
  lens = torch.tensor(lens_h, dtype=torch.int32, device=cuda)
  xh = torch.randn((3, 50, 64)).to(torch.bfloat16)
  for b, n in enumerate(lens_h):
    xh[b, n:] = 0
  x = Act(xh.to(cuda), lens, requires_grad=False)
  lens2 = (lens + 1) // 2

  def run(L, training=False, tape=None):
    return conv_bn_actv(L, x, lens if L is layer else lens2, "relu", training, tape).data

  def model():                                          # quantise -> conv -> affine -> ReLU -> mask, in fp64
    _, _, x_deq = _mx_ref(xh.view(150, 64))
    _, _, w_deq = _mx_ref(layer.kernel.w16.cpu().view(11 * 128, 64))
    cs = layer.gamma.master.cpu().double() / (layer.moving_var.cpu().double() + layer.eps).sqrt()
    cb = layer.beta.master.cpu().double() - layer.moving_mean.cpu().double() * cs
    return _conv_ref(x_deq.view(3, 50, 64), w_deq.view(11, 128, 64), 1, 5, lens_h, cs, cb, 1, lens_h)
  bf16, bf16_tape, bf16_twin = run(layer), run(layer, tape=Tape()), run(twin)
  layer.mxfp8 = twin.mxfp8 = True
  y = run(layer)
  _check(y, *model())
  assert not torch.equal(y, bf16)                       # it is the other path
  assert torch.equal(run(layer, tape=Tape()), bf16_tape) and torch.equal(run(twin), bf16_twin)
  # the weight copy follows the store's version counter
  layer.kernel.master.mul_(2.0)
  store.refresh_compute_copies()
  _check(run(layer), *model())
  # training (batch statistics; last, it moves the moving statistics) keeps the bf16 path
  layer.mxfp8 = False
  train_bf16 = run(layer, training=True)
  layer.mxfp8 = True
  assert torch.equal(run(layer, training=True), train_bf16)


def test_encoder_switch(cuda):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.tdnn_encoder import TDNNEncoder
  # the convnet_layers of jasper_res_blockout_test_config.py; 64 features instead of 40 (a multiple of 64) and plain
  # ReLU instead of the clipped one (the MXFP8 path takes ReLU / none, a clipped ReLU keeps every layer on bf16)
  conv = lambda **kw: dict(type="conv1d", stride=[1], padding="SAME", dilation=[1], **kw)
  layers = [conv(repeat=1, kernel_size=[7], num_channels=128), conv(repeat=2, kernel_size=[7], num_channels=256,
            residual=True), conv(repeat=2, kernel_size=[1], num_channels=256, residual=True)]

  def run(**extra):
    torch.manual_seed(0)
    store = FlatParams(cuda)
    enc = TDNNEncoder(dict({"convnet_layers": layers, "dropout_keep_prob": 0.9, "activation_fn": "relu",
                            "drop_block_prob": 0.2, "drop_block_index": -1, "use_conv_mask": True,
                            "dtype": "mixed"}, **extra), None, mode="eval").build(store, 64)
    store.finalize()
    g = torch.Generator().manual_seed(5)
    x = torch.randn((4, 300, 64), generator=g).to(torch.bfloat16).to(cuda)
    lens = torch.tensor([300, 257, 120, 9], dtype=torch.int32, device=cuda)
    return enc.encode({"source_tensors": [x, lens]})["outputs"]
  off, on = run().float(), run(mxfp8_inference=True).float()      # the bf16 path is the parent's behaviour
  assert bool(torch.isfinite(on).all())
  rel = float((on - off).norm() / off.norm())
  print("encoder rel L2 (mxfp8 vs bf16) = %.4g" % rel)
  assert 0.0 < rel < ENCODER_REL_L2_BOUND
