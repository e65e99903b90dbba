"""The RNN NMT model of tests/test_nmt_e2e_gpu.py::test_nmt_small_fwd_bwd (2-layer bidirectional LSTM encoder with
embedding -> gnmt_v2 attention decoder -> BasicSequenceLoss; V 30, E 64, H 64, B 4, S 11, T 9) at attention
widths the decoder loop used to refuse: attention_layer_size 1024 (the en-de-gnmt-like configs) and 200 (no
multiple of 128). Same tolerances against oracle/nmt.py: encoder outputs 3e-2, logits 5e-2, loss rel 2e-2, every
parameter gradient cos > 0.99 and rel < 0.12. The kernels guard the partial last 128-block themselves, so no
variable is padded: the stored attention variables have the logical width.

Long sources: the same model at width 128 on one batch with src_len = [300, 1, 150, 40] — beam decoding in
infer mode returns finite scores and lengths >= 1, and the teacher-forced logits match the oracle at 5e-2."""
import pytest
import torch

from test_nmt_e2e_gpu import _cmp, _oracle_params

pytestmark = pytest.mark.gpu

V, E, H, LAYERS, B = 30, 64, 64, 2, 4


def _build(cuda, width, mode="train", decoder=None, extra=None):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders import BidirectionalRNNEncoderWithEmbedding
  from openseq2seq_amd.decoders import RNNDecoderWithAttention
  from openseq2seq_amd.losses import BasicSequenceLoss
  store = FlatParams(cuda)
  cellp = {"num_units": H, "forget_bias": 1.0}
  enc = BidirectionalRNNEncoderWithEmbedding(
      {"src_vocab_size": V, "src_emb_size": E, "encoder_layers": LAYERS,
       "encoder_use_skip_connections": False, "core_cell": "LSTMCell", "core_cell_params": cellp,
       "encoder_dp_input_keep_prob": 1.0, "dtype": "mixed"}, None, mode=mode).build(store)
  dec = (decoder or RNNDecoderWithAttention)(
      dict({"GO_SYMBOL": 2, "END_SYMBOL": 1, "tgt_vocab_size": V, "tgt_emb_size": E,
            "attention_layer_size": width, "attention_type": "gnmt_v2", "core_cell": "LSTMCell",
            "core_cell_params": cellp, "decoder_layers": LAYERS, "decoder_use_skip_connections": False,
            "decoder_dp_input_keep_prob": 1.0, "batch_size": B, "dtype": "mixed"}, **(extra or {})), None, mode=mode)
  dec.build(store, memory_dim=2 * H)
  loss = BasicSequenceLoss({"tgt_vocab_size": V, "batch_size": B, "offset_target_by_one": True,
                            "average_across_timestep": False, "do_mask": True, "dtype": "mixed"}, None)
  store.finalize()
  return store, enc, dec, loss


def _perturb(store, cuda, g):
  for p in store.params:      # non-trivial biases / attention vectors
    if p.kind == "vector" and p.numel > 1:
      p.master.add_((torch.randn(p.shape, generator=g) * 0.1).to(cuda))
  store.refresh_compute_copies()


def _batch(g, src_len, tgt_len):
  S, T = int(src_len.max()), int(tgt_len.max())
  src = torch.randint(4, V, (B, S), generator=g).to(torch.int32)
  tgt = torch.randint(4, V, (B, T), generator=g).to(torch.int32)
  for b in range(B):
    src[b, src_len[b]:] = 0
    tgt[b, 0] = 2
    tgt[b, tgt_len[b] - 1] = 1
    tgt[b, tgt_len[b]:] = 0
  return src, tgt


@pytest.mark.parametrize("width", [1024, 200])
def test_nmt_wide_attention_fwd_bwd(cuda, width):
  from openseq2seq_amd.parts.cnns.conv_blocks import Tape
  from openseq2seq_amd.parts.transformer.layers import SeedSeq
  from oracle import nmt as onmt
  torch.manual_seed(0)
  store, enc, dec, lossf = _build(cuda, width)
  c = dec.cell
  assert c.U == width and tuple(c.v.shape) == (width,) and tuple(c.b.shape) == (width,)
  assert tuple(c.w_q.shape) == (1, width, H) and tuple(c.w_mem.shape) == (1, width, 2 * H)
  g = torch.Generator().manual_seed(1)
  _perturb(store, cuda, g)
  src_len = torch.tensor([11, 6, 9, 3], dtype=torch.int32)
  tgt_len = torch.tensor([9, 4, 7, 2], dtype=torch.int32)
  T = 9
  src, tgt = _batch(g, src_len, tgt_len)
  tape = Tape()
  store.zero_grads()
  e = enc.encode({"source_tensors": [src.to(cuda), src_len.to(cuda)], "tape": tape, "seeds": SeedSeq(3)})
  d = dec.decode({"encoder_output": e, "target_tensors": [tgt.to(cuda), tgt_len.to(cuda)], "tape": tape})
  L = lossf.compute_loss({"decoder_output": d, "target_tensors": [tgt.to(cuda), tgt_len.to(cuda)]})
  tape.backward()
  torch.cuda.synchronize()
  P, D, leaves = _oracle_params(store, enc, dec, V)
  enc_out = onmt.encoder(P, src, src_len)
  logits = onmt.decoder_logits(D, enc_out, src_len, tgt, tgt_len, "gnmt_v2")[..., :V]
  ref = onmt.basic_sequence_loss(logits, tgt, tgt_len, B)
  ref.backward()
  torch.testing.assert_close(e["outputs"].float().cpu(), enc_out.detach(), atol=3e-2, rtol=3e-2)
  live = (torch.arange(T)[None, :] < tgt_len[:, None])
  got_logits = d["logits"].float().cpu()[..., :V]
  torch.testing.assert_close(got_logits[live], logits.detach()[live], atol=5e-2, rtol=5e-2)
  assert abs(float(L.item()) - float(ref)) <= 2e-2 * abs(float(ref)), (float(L.item()), float(ref))
  bad = []
  for p in store.params:
    gref = leaves[p.name].grad
    if gref is None:
      gref = torch.zeros_like(leaves[p.name])
    try:
      _cmp(p.grad.reshape(-1), gref.reshape(-1), p.name)
    except AssertionError as ex:
      bad.append(ex.args[0])
  assert not bad, bad


def test_nmt_long_source(cuda):
  from openseq2seq_amd.decoders import BeamSearchRNNDecoderWithAttention
  from oracle import nmt as onmt
  torch.manual_seed(0)
  store, enc, dec, _ = _build(cuda, 128)
  g = torch.Generator().manual_seed(1)
  _perturb(store, cuda, g)
  src_len = torch.tensor([300, 1, 150, 40], dtype=torch.int32)
  tgt_len = torch.tensor([9, 4, 7, 2], dtype=torch.int32)
  T = 9
  src, tgt = _batch(g, src_len, tgt_len)
  # teacher-forced forward against the oracle
  e = enc.encode({"source_tensors": [src.to(cuda), src_len.to(cuda)], "tape": None})
  d = dec.decode({"encoder_output": e, "target_tensors": [tgt.to(cuda), tgt_len.to(cuda)], "tape": None})
  P, D, _ = _oracle_params(store, enc, dec, V)
  with torch.no_grad():
    enc_out = onmt.encoder(P, src, src_len)
    logits = onmt.decoder_logits(D, enc_out, src_len, tgt, tgt_len, "gnmt_v2")[..., :V]
  live = (torch.arange(T)[None, :] < tgt_len[:, None])
  torch.testing.assert_close(d["logits"].float().cpu()[..., :V][live], logits[live], atol=5e-2, rtol=5e-2)
  # beam decoding of the same variables in infer mode
  store2, enc2, dec2, _ = _build(cuda, 128, mode="infer", decoder=BeamSearchRNNDecoderWithAttention,
                                 extra={"beam_width": 3, "length_penalty": 1.0})
  assert [p.name for p in store2.params] == [p.name for p in store.params]
  store2.master.copy_(store.master)
  store2.refresh_compute_copies()
  e2 = enc2.encode({"source_tensors": [src.to(cuda), src_len.to(cuda)]})
  o = dec2.decode({"encoder_output": e2})
  torch.cuda.synchronize()
  assert o["predicted_ids"].shape[0] == B and o["predicted_ids"].shape[2] == 3
  assert bool(torch.isfinite(o["scores"]).all()), o["scores"]
  lens = o["final_sequence_lengths"].cpu()
  assert bool((lens >= 1).all()) and int(lens.max()) <= 2 * 300, lens


@pytest.mark.parametrize("weight_tied", [False, True])
def test_gnmt_like_config_train_eval_infer(cuda, weight_tied):
  """configs.nmt.gnmt_like_config (en-de-gnmt-like-4GPUs.py / -weight-tied-2GPUs.py) scaled down to 64 units —
  attention_layer_size 64, below the old 128 granule — runs a train step, a greedy eval pass and a beam-search
  infer on synthetic batches."""
  import copy
  from openseq2seq_amd.configs.nmt import gnmt_like_config
  from openseq2seq_amd.decoders import BeamSearchRNNDecoderWithAttention
  cls, params = gnmt_like_config(batch_size_per_gpu=4, vocab=96, weight_tied=weight_tied, units=64,
                                 encoder_layers=3, decoder_layers=3, max_length=12)
  assert params["decoder_params"]["attention_layer_size"] == 64
  train = cls(copy.deepcopy(params), mode="train", hvd=None, device=cuda)
  train.compile()
  batch = train.get_data_layer().synthetic_batch(cuda, seed=3, fixed_len=9)
  loss = train.train_step(batch)
  assert bool(torch.isfinite(loss.cpu()).all())
  ev = cls(copy.deepcopy(params), mode="eval", hvd=None, device=cuda)
  ev.compile()
  ids, lens = ev.infer_batch(batch)
  assert ids.shape[0] == 4 and bool((lens.cpu() >= 1).all())
  p2 = copy.deepcopy(params)
  p2["decoder"] = BeamSearchRNNDecoderWithAttention
  p2["decoder_params"] = dict(p2["decoder_params"], beam_width=3, length_penalty=1.0)
  bs = cls(p2, mode="infer", hvd=None, device=cuda)
  bs.compile()
  ids, lens = bs.infer_batch(batch)
  torch.cuda.synchronize()
  assert ids.shape[0] == 4 and bool((lens.cpu() >= 1).all()) and int(lens.max()) <= 18
