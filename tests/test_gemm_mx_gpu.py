"""MXFP8 inference path (csrc/gemm_mx.hip): the quantiser bit for bit against the format rule restated here, the
block-scaled GEMM against the fp64 product of the dequantised operands within the worst-case fp32 summation bound,
the refusals of the C ABI, and the 'mxfp8_inference' switch of Dense / TransformerEncoder."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# relative L2 distance of the toy encoder's MXFP8 output to its bf16 output: 3 x the value measured on an MI355X
# (profiles/mxfp8_first_measurements.md); a broken layer shows as O(1)
ENCODER_REL_L2_MEASURED = 0.04133
ENCODER_REL_L2_BOUND = 3 * ENCODER_REL_L2_MEASURED


def _mx_ref(x):
  """The format rule on the CPU. x: bf16 [rows, K] -> (e4m3 bytes [rows, K], scale bytes [rows, K / 32], the
  dequantised values in fp64). e = floor(log2(amax)) - 8, byte = clamp(e + 127, 0, 254), element = RNE(clamp(x 2^-e))."""
  rows, K = x.shape
  xb = x.double().view(rows, K // 32, 32)
  amax = xb.abs().amax(-1)
  _, ex = torch.frexp(amax)                         # amax = m 2^ex, m in [0.5, 1): floor(log2) = ex - 1
  byte = torch.where(amax > 0, (ex - 1 - 8 + 127).clamp(0, 254), torch.zeros_like(ex)).to(torch.int32)
  scaled = torch.ldexp(xb, (127 - byte)[..., None]).clamp(-448.0, 448.0).float()
  q = scaled.to(torch.float8_e4m3fn)
  deq = torch.ldexp(q.double(), (byte - 127)[..., None]).view(rows, K)
  return q.view(torch.uint8).view(rows, K), byte.to(torch.uint8), deq


def _device_scales(sb, K):
  """[rows, K / 32] scale bytes -> the [ceil(K / 128), rows, 4] layout of os2s.h (zeros past K)."""
  rows, KT = sb.shape[0], (K + 127) // 128
  pad = torch.zeros((rows, KT * 4), dtype=torch.uint8)
  pad[:, :K // 32] = sb
  return pad.view(rows, KT, 4).permute(1, 0, 2).contiguous()


@pytest.mark.parametrize("rows,K,strided", [(1, 64, False), (33, 64, False), (33, 96 * 32, False),
                                            (1, 96 * 32, True), (33, 64, True)])
def test_quantiser_bit_exact(cuda, rows, K, strided):
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(rows * 7 + K)
  ld = K + 24 if strided else K
  buf = (torch.randn((rows, ld), generator=g) * torch.exp2(torch.randint(-9, 9, (rows, ld), generator=g).float()))
  x = buf.to(torch.bfloat16)[:, :K].contiguous()
  special = [torch.tensor([-15.0, 7.5] * 16),                          # 15 = 1.875 * 8: scaled amax 480, saturates
             torch.zeros(32),                                          # all zero
             torch.tensor([4.0, -4.0, 3.0, -0.015625] * 8),            # amax an exact power of two, both signs
             torch.tensor([2.0 ** -20, -(2.0 ** -22)] * 16),           # tiny ...
             torch.tensor([2.0 ** 20, -1.5 * 2.0 ** 19] * 16)]         # ... next to huge
  for i, s in enumerate(special[:rows * K // 32]):
    r, b = divmod(i, K // 32)
    x[r, b * 32:(b + 1) * 32] = s.to(torch.bfloat16)
  if strided:
    full = torch.zeros((rows, ld), dtype=torch.bfloat16)
    full[:, :K] = x
    xd = full.to(cuda)[:, :K]
  else:
    xd = x.to(cuda)
  q_ref, s_ref, _ = _mx_ref(x)
  assert int((q_ref & 0x7f).max()) == 0x7e and 0x7f not in (q_ref & 0x7f)      # 448 is reached, NaN never
  q, sc = capi.quantize_mx(xd)
  assert torch.equal(capi.mx_scales_by_row(sc, K).cpu(), s_ref)
  assert torch.equal(q.cpu(), q_ref)


def _operand(rows, K, g, shift):
  """Every (row, K block) has its own power-of-two magnitude: a misrouted scale moves an output by 2x or more."""
  r = torch.arange(rows)[:, None]
  b = torch.arange(K // 32)[None, :]
  mag = torch.exp2(((r + 3 * b + shift) % 13 - 6).float()).repeat_interleave(32, dim=1)
  mant = 1.0 + torch.rand((rows, K), generator=g)
  sign = torch.where(torch.rand((rows, K), generator=g) < 0.5, -1.0, 1.0)
  return (mag * mant * sign).to(torch.bfloat16)


def _gemm_ref(a_deq, w_deq, bias=None, act=0, residual=None, out_f32=False):
  """(fp64 reference, elementwise bound): K 2^-22 sum |a||w| — worst-case fp32 summation with one bit for a
  truncating accumulator — plus 2^-8 |ref| for a bf16 result."""
  K = a_deq.shape[1]
  ref = a_deq @ w_deq.t()
  if bias is not None:
    ref = ref + bias.double()
  if act == 1:
    ref = ref.clamp_min(0.0)
  if residual is not None:
    ref = ref + residual.double()
  bound = K * 2.0 ** -22 * (a_deq.abs() @ w_deq.abs().t())
  if not out_f32:
    bound = bound + 2.0 ** -8 * ref.abs()
  return ref, bound


def _check(out, ref, bound):
  err = (out.double().cpu() - ref).abs()
  print("max err / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
  assert bool((err <= bound).all())


@pytest.mark.parametrize("M,N,K,epi,strided", [
    (1, 8, 64, "none", False), (33, 264, 192, "bias_relu", False), (257, 264, 1024, "bias_res", False),
    (257, 8, 192, "f32", False), (33, 8, 1024, "none", False), (1, 264, 1024, "bias_relu", False),
    (257, 264, 64, "f32", False), (33, 264, 64, "bias_res", True), (257, 8, 64, "bias_relu", False),
    (1, 264, 192, "bias_res", False), (33, 8, 192, "f32", False), (257, 264, 192, "none", False)])
def test_gemm_against_fp64(cuda, M, N, K, epi, strided):
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(M + 3 * N + 5 * K)
  aq, asb, a_deq = _mx_ref(_operand(M, K, g, 0))
  wq, wsb, w_deq = _mx_ref(_operand(N, K, g, 5))
  bias = torch.randn(N, generator=g) if epi in ("bias_relu", "bias_res") else None
  res = torch.randn((M, N), generator=g).to(torch.bfloat16) if epi == "bias_res" else None
  act, f32 = int(epi == "bias_relu"), epi == "f32"
  if strided:
    wide = torch.zeros((M, K + 48), dtype=torch.uint8)
    wide[:, :K] = aq
    aq_d = wide.to(cuda)[:, :K]
  else:
    aq_d = aq.to(cuda)
  out = capi.gemm_nt_mx(aq_d, _device_scales(asb, K).to(cuda), wq.to(cuda), _device_scales(wsb, K).to(cuda),
                        bias=bias.to(cuda) if bias is not None else None, act=act,
                        residual=res.to(cuda) if res is not None else None, out_f32=f32)
  assert out.dtype == (torch.float32 if f32 else torch.bfloat16)
  _check(out, *_gemm_ref(a_deq, w_deq, bias, act, res, f32))


def test_refusals(cuda):
  from openseq2seq_amd import _lib
  f = _lib.lib().os2s_gemm_nt_mx                      # the library's own attribute: returns the status
  t = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
  p = t.data_ptr()

  def call(a, M, N, K):
    return f(None, a, K, p, p, p, p, N, M, N, K, None, 0, None, 0)
  assert call(p, 16, 64, 64) == 0
  assert call(p, 16, 64, 72) == -3                    # OS2S_ERR_UNSUPPORTED
  assert call(p, 16, 12, 64) == -3
  assert call(None, 16, 64, 64) == -1                 # OS2S_ERR_INVALID_ARG
  torch.cuda.synchronize()


def test_dense_switch(cuda):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.parts.dense import Dense
  from openseq2seq_amd.parts.tape import Act, Tape
  torch.manual_seed(3)
  store = FlatParams(cuda)
  d = Dense(store, "d", 128, 512, True)
  store.finalize()
  d.bias.master.copy_(torch.randn(512))
  x = torch.randn((600, 128)).to(torch.bfloat16)
  xa = lambda rows: Act(x[:rows].to(cuda), requires_grad=False)
  bf16 = d.forward(xa(600), None).data
  bf16_tape = d.forward(xa(600), Tape()).data
  bf16_skinny = d.forward(xa(8), None).data
  d.mxfp8 = True
  y = d.forward(xa(600), None).data
  _, _, a_deq = _mx_ref(x)
  _, _, w_deq = _mx_ref(d.w.cpu())
  _check(y, *_gemm_ref(a_deq, w_deq, d.bias.master.cpu()))
  assert not torch.equal(y, bf16)                     # it is the other path
  assert torch.equal(d.forward(xa(600), Tape()).data, bf16_tape)
  assert torch.equal(d.forward(xa(8), None).data, bf16_skinny)
  # the weight copy follows the store's version counter
  d.kernel.master.mul_(2.0)
  store.refresh_compute_copies()
  _, _, w_deq = _mx_ref(d.w.cpu())
  _check(d.forward(xa(600), None).data, *_gemm_ref(a_deq, w_deq, d.bias.master.cpu()))


def test_encoder_switch(cuda):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.transformer_encoder import TransformerEncoder

  def run(**extra):                                   # the encoder of nmt-reversal-TT.py, eval mode
    torch.manual_seed(0)
    store = FlatParams(cuda)
    enc = TransformerEncoder(dict({"encoder_layers": 2, "hidden_size": 128, "num_heads": 8, "attention_dropout": 0.1,
                                   "filter_size": 512, "src_vocab_size": 24, "relu_dropout": 0.1,
                                   "layer_postprocess_dropout": 0.1, "remove_padding": True, "dtype": "mixed"},
                                  **extra), None, mode="eval").build(store)
    store.finalize()
    rng = np.random.RandomState(5)
    ids = rng.randint(4, 24, size=(32, 24)).astype(np.int32)      # 768 tokens: above the skinny kernel's rows
    lens = np.full((32,), 24, np.int32)
    return enc.encode({"source_tensors": [torch.from_numpy(ids).to(cuda), torch.from_numpy(lens).to(cuda)]})["outputs"]
  off, on = run().float(), run(mxfp8_inference=True).float()
  assert bool(torch.isfinite(on).all())
  rel = float((on - off).norm() / off.norm())
  print("encoder rel L2 (mxfp8 vs bf16) = %.4g" % rel)
  assert 0.0 < rel < ENCODER_REL_L2_BOUND
