"""MXFP8 decode-step GEMM (csrc/gemm_skinny_mx.hip): every tile variant against the fp64 product of the operands
quantised by the format rule restated here (the in-kernel quantiser has to follow it bit for bit to stay inside the
fp32 summation bound), the refusals of the C ABI, and the 'mxfp8_decode' switch of Dense / TransformerDecoder."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# relative L2 distance of one toy decode step's MXFP8 logits to its bf16 logits: 3 x the value measured on an MI355X
# (profiles/mxfp8_decode_first_measurements.md); a broken layer shows as O(1)
STEP_REL_L2_MEASURED = 0.02483
STEP_REL_L2_BOUND = 3 * STEP_REL_L2_MEASURED


def _mx_ref(x):
  """The format rule on the CPU (as tests/test_gemm_mx_gpu.py). x: bf16 [rows, K] -> (e4m3 bytes [rows, K], scale
  bytes [rows, K / 32], the dequantised values in fp64). e = floor(log2(amax)) - 8, byte = clamp(e + 127, 0, 254),
  element = RNE(clamp(x 2^-e))."""
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


def _operand(rows, K, g, shift):
  """Every (row, K block) has its own power-of-two magnitude: a misrouted scale moves an output by 2x or more."""
  r = torch.arange(rows)[:, None]
  b = torch.arange(K // 32)[None, :]
  mag = torch.exp2(((r + 3 * b + shift) % 13 - 6).float()).repeat_interleave(32, dim=1)
  mant = 1.0 + torch.rand((rows, K), generator=g)
  sign = torch.where(torch.rand((rows, K), generator=g) < 0.5, -1.0, 1.0)
  return (mag * mant * sign).to(torch.bfloat16)


def _check(out, x, w_deq, bias=None, relu=False, residual=None):
  """|out - fp64 reference| <= K 2^-22 sum |a||w| (worst-case fp32 summation, one bit for a truncating
  accumulator) + 2^-8 |ref| (bf16 result), elementwise; a = the format rule applied to x."""
  a_deq = _mx_ref(x)[2]
  ref = a_deq @ w_deq.t()
  if bias is not None:
    ref = ref + bias.double()
  if relu:
    ref = ref.clamp_min(0.0)
  if residual is not None:
    ref = ref + residual.double()
  bound = x.shape[1] * 2.0 ** -22 * (a_deq.abs() @ w_deq.abs().t()) + 2.0 ** -8 * ref.abs()
  err = (out.double().cpu() - ref).abs()
  print("max err / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
  assert bool((err <= bound).all())


# tile: 0 = 32x32, 1 = 64x64, 2 = 64x128, 3 = 128x256, 4 = 256x256 (m x n), -1 = by shape
@pytest.mark.parametrize("tile,M,N,K,epi,strided", [
    (0, 1, 8, 64, "none", False), (0, 33, 264, 1024, "bias_relu", False), (0, 65, 264, 192, "bias_res", True),
    (1, 65, 264, 1024, "bias_res", False), (1, 33, 8, 192, "bias_relu", False), (1, 1, 264, 64, "none", True),
    (2, 65, 264, 1024, "bias_relu", False), (2, 33, 264, 192, "none", False), (2, 1, 8, 64, "bias_res", False),
    (3, 65, 264, 1024, "none", False), (3, 33, 264, 192, "bias_res", False), (3, 1, 8, 64, "bias_relu", False),
    (4, 65, 264, 1024, "bias_res", False), (4, 33, 8, 192, "bias_relu", True), (4, 1, 264, 64, "none", False),
    (-1, 65, 264, 1024, "bias_relu", False), (-1, 33, 264, 192, "bias_res", False)])
def test_kernel_against_fp64(cuda, tile, M, N, K, epi, strided):
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(M + 3 * N + 5 * K)
  x = _operand(M, K, g, 0)
  wq, wsb, w_deq = _mx_ref(_operand(N, K, g, 5))
  bias = torch.randn(N, generator=g) if epi != "none" else None
  res = torch.randn((M, N), generator=g).to(torch.bfloat16) if epi == "bias_res" else None
  if strided:
    wide = torch.zeros((M, K + 24), dtype=torch.bfloat16)
    wide[:, :K] = x
    xd = wide.to(cuda)[:, :K]
  else:
    xd = x.to(cuda)
  run = lambda: capi.gemm_skinny_mx(xd, wq.to(cuda), _device_scales(wsb, K).to(cuda),
                                    bias=bias.to(cuda) if bias is not None else None, relu=(epi == "bias_relu"),
                                    residual=res.to(cuda) if res is not None else None, tile=tile)
  out, again = run(), run()
  assert out.dtype == torch.bfloat16 and torch.equal(out, again)      # K-shares are reduced in a fixed order
  _check(out, x, w_deq, bias, epi == "bias_relu", res)


def test_refusals(cuda):
  from openseq2seq_amd import _lib
  f = _lib.lib().os2s_gemm_skinny_mx                  # the library's own attribute: returns the status
  t = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
  p = t.data_ptr()

  def call(x, M, N, K):
    return f(None, x, K, p, p, None, None, 0, M, N, K, 0, p, N, -1)
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
  x = torch.randn((64, 128)).to(torch.bfloat16)
  xa = lambda rows: Act(x[:rows].to(cuda), requires_grad=False)
  bf16 = {rows: d.forward(xa(rows), None).data for rows in (8, 64)}
  bf16_tape = d.forward(xa(64), Tape()).data
  d.mxfp8_decode = True
  w_deq = _mx_ref(d.w.cpu())[2]
  for rows in (8, 64):
    y = d.forward(xa(rows), None).data
    _check(y, x[:rows], w_deq, d.bias.master.cpu())
    assert not torch.equal(y, bf16[rows])             # it is the other path
  assert torch.equal(d.forward(xa(64), Tape()).data, bf16_tape)
  d.mxfp8_decode = False
  assert all(torch.equal(d.forward(xa(rows), None).data, bf16[rows]) for rows in (8, 64))
  # the weight copy follows the store's version counter
  d.mxfp8_decode = True
  d.kernel.master.mul_(2.0)
  store.refresh_compute_copies()
  _check(d.forward(xa(64), None).data, x, _mx_ref(d.w.cpu())[2], d.bias.master.cpu())


def _toy(cuda, **extra):
  """Encoder output and decoder of nmt-reversal-TT.py sizes, infer mode; the same weights for the same seed."""
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.transformer_encoder import TransformerEncoder
  from openseq2seq_amd.decoders.transformer_decoder import TransformerDecoder
  torch.manual_seed(3)
  store = FlatParams(cuda)
  common = {"hidden_size": 128, "num_heads": 8, "attention_dropout": 0.1, "filter_size": 512, "relu_dropout": 0.1,
            "layer_postprocess_dropout": 0.1, "dtype": "mixed"}
  enc = TransformerEncoder(dict(common, encoder_layers=2, src_vocab_size=40, remove_padding=True), None,
                           mode="infer").build(store)
  dec = TransformerDecoder(dict(common, EOS_ID=1, num_hidden_layers=2, batch_size=5, tgt_vocab_size=40, beam_size=4,
                                alpha=0.6, extra_decode_length=6, **extra), None, mode="infer").build(store)
  store.finalize()
  # sharpen the output distribution so that beams are well separated
  emb = store.by_name("ForwardPass/transformer_encoder/embedding_shared_weights/embedding_and_softmax/weights")
  emb.master.mul_(4.0)
  store.refresh_compute_copies()
  rng = np.random.RandomState(2)
  ids = rng.randint(4, 40, size=(5, 9)).astype(np.int32)
  ids[:, -1] = 1
  lens = np.full((5,), 9, np.int32)
  return enc.encode({"source_tensors": [torch.from_numpy(ids).to(cuda), torch.from_numpy(lens).to(cuda)]}), dec


def test_beam_search_switch(cuda):
  e, dec = _toy(cuda, mxfp8_decode=True)
  out = dec.decode({"encoder_output": e})
  eager = dec.decode({"encoder_output": e, "use_graph": False})
  # the hipGraph-replayed loop and the eager loop run the same kernels on the same cached weight copies
  assert torch.equal(eager["outputs"][0], out["outputs"][0]) and torch.equal(eager["scores"], out["scores"])
  assert bool(torch.isfinite(out["scores"]).all())

  def step_logits(e, dec):            # the third step of five beam rows fed fixed ids
    fn = dec._get_symbols_to_logits_fn(e, 1, 5, 4)
    cache = {"ancestry": torch.zeros((5, 4), dtype=torch.int32, device=cuda)}
    ids = torch.tensor([[0, 7, 21, 13]] * 5, dtype=torch.int32, device=cuda) + torch.arange(5, device=cuda)[:, None].int()
    ids[:, 0] = 0
    for i in range(3):
      logits, cache = fn(ids[:, :i + 1], i, cache)
    return logits.float()
  on = step_logits(e, dec)
  off = step_logits(*_toy(cuda))
  rel = float((on - off).norm() / off.norm())
  print("decode step rel L2 (mxfp8_decode vs bf16) = %.4g" % rel)
  assert 0.0 < rel < STEP_REL_L2_BOUND
