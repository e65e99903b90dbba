"""LMEncoder with use_cudnn_rnn (lstm-test-small-cudnn.py: CudnnLSTM of emb_size units on the existing cuDNN-form
LSTM kernels): a train step gives a finite loss near ln V and a gradient for every variable; generation, which re-runs
the growing prefix each step (those kernels take no initial state), gives the argmax of the eval-mode logits over
the same prefix."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

V, E, B, T = 17, 16, 3, 5


def _params(**over):
  p = dict(vocab_size=V, emb_size=E, encoder_layers=2, encoder_use_skip_connections=False, core_cell=None,
           core_cell_params=dict(num_units=32, forget_bias=1.0), end_token=V + 3, batch_size=B, use_cudnn_rnn=True,
           cudnn_rnn_type="CudnnLSTM", encoder_dp_input_keep_prob=1.0, encoder_dp_output_keep_prob=1.0,
           recurrent_keep_prob=1.0, encoder_emb_keep_prob=1.0, fc_use_bias=True, weight_tied=True, dtype="float32")
  p.update(over)
  return p


def _build(cuda, mode, **over):
  from openseq2seq_amd.encoders import LMEncoder
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  torch.manual_seed(5)
  store = FlatParams(cuda)
  enc = LMEncoder(_params(**over), None, mode=mode).build(store)
  store.finalize()
  return store, enc


def test_cudnn_lm_trains_and_generates(cuda):
  from openseq2seq_amd.losses import BasicSequenceLoss
  from openseq2seq_amd.parts.tape import Tape
  store, enc = _build(cuda, "train")
  lossf = BasicSequenceLoss(dict(tgt_vocab_size=V, batch_size=B, offset_target_by_one=False,
                                 average_across_timestep=True, do_mask=False), None)
  g = torch.Generator().manual_seed(1)
  stream = torch.randint(0, V, (B, T + 1), generator=g, dtype=torch.int32).to(cuda)
  lens = torch.full((B,), T, dtype=torch.int32, device=cuda)
  tape = Tape()
  store.zero_grads()
  e = enc.encode({"source_tensors": [stream[:, :-1].contiguous(), lens], "tape": tape})
  L = lossf.compute_loss({"decoder_output": e, "target_tensors": [stream[:, 1:].contiguous(), lens]})
  tape.backward()
  torch.cuda.synchronize()
  assert abs(float(L.cpu()[0]) - math.log(V)) < 0.5
  for p in store.params:
    assert bool(torch.isfinite(p.grad).all()) and (float(p.grad.abs().max()) > 0.0 or p.name.endswith("bias_h")), p.name
  seeds = [2, 9]
  store_i, gen = _build(cuda, "infer", seed_tokens=seeds, num_tokens_gen=4)
  store_i.master.copy_(store.master)
  store_i.refresh_compute_copies()
  out = gen.encode({"source_tensors": [None, None]})
  ids = out["outputs"][0].cpu()
  assert ids.shape == (2, 4)
  store_e, ev = _build(cuda, "eval", batch_size=2)
  store_e.master.copy_(store.master)
  store_e.refresh_compute_copies()
  prefix = torch.cat([torch.tensor(seeds, dtype=torch.int32).view(2, 1), ids[:, :-1].to(torch.int32)], dim=1).to(cuda)
  full = ev.encode({"source_tensors": [prefix, torch.full((2,), 4, dtype=torch.int32, device=cuda)]})
  assert torch.equal(full["logits"][:, :, :V].float().cpu().argmax(dim=2), ids.long())
