"""The Transformer training path on sentences longer than 64 tokens: every attention of the encoder and decoder
(self, causal self, encoder-decoder) goes through the tile-walking kernels of csrc/attention_long.hpp. Loss, logits
and parameter gradients against the CPU fp32 oracle with the tolerances of test_transformer_small_fwd_bwd
(tests/test_transformer_e2e_gpu.py), and the training loop of test_transformer_small_trains."""
import numpy as np
import pytest
import torch

import _transformer_long_cases as C

pytestmark = pytest.mark.gpu

SRC_LENS = [150, 65, 64, 9]
TGT_LENS = [129, 3, 70, 128]
TOL = dict(loss=2e-2, logits=3e-2, cos=0.98, rel=0.2)


@pytest.mark.parametrize("dims", [(512, 8, 1024, 1000, 2), (256, 8, 512, 1000, 2)], ids=["dh64", "dh32"])
def test_transformer_long_fwd_bwd(cuda, dims):
  C.fwd_bwd(cuda, dims, SRC_LENS, TGT_LENS, TOL)


def test_transformer_long_trains(cuda):
  """40 LazyAdam steps on one fixed batch of 8 sentence pairs of 70-140 tokens, dropout 0.1 (attention dropout
  through the multi-tile forward and backward). Measured on an MI355X: loss 11.35 -> 4.97, ratio 0.44, no skipped
  step; the short-sentence test's 0.6 is asserted here too."""
  from openseq2seq_amd.parts.cnns.conv_blocks import Tape
  from openseq2seq_amd.parts.transformer.layers import SeedSeq
  from openseq2seq_amd.optimizers.optimizers import optimize_loss
  from openseq2seq_amd.optimizers import lr_policies
  dims = (512, 8, 1024, 1000, 2)
  store, enc, dec, lossf = C.build(cuda, dims, dropout=0.1)
  op = optimize_loss(store, "LazyAdam", dict(beta1=0.9, beta2=0.997, epsilon=1e-9),
                     lr_policies.transformer_policy,
                     dict(learning_rate=2.0, warmup_steps=40, d_model=dims[0]), loss_scaling="Backoff")
  rng = np.random.RandomState(5)
  batch, *_ = C.batch_of(cuda, rng.randint(70, 141, size=8), rng.randint(70, 141, size=8), dims[3], seed=5)
  losses = []
  for step in range(40):
    tape = Tape()
    store.zero_grads()
    e = enc.encode({'source_tensors': batch['source_tensors'], 'tape': tape,
                    'seeds': SeedSeq(step + 1), 'packed_source': batch['packed_source']})
    d = dec.decode({'encoder_output': e, 'target_tensors': batch['target_tensors'], 'tape': tape,
                    'packed_target': batch['packed_target']})
    L = lossf.compute_loss({'decoder_output': d, 'target_tensors': batch['target_tensors'],
                            'loss_scale_dev': op.loss_scale_view})
    tape.backward()
    op.run()
    losses.append(float(L.cpu()[0]))
  st = op.read_state()
  print("losses first / last / ratio", losses[0], losses[-1], losses[-1] / losses[0])
  assert np.isfinite(losses).all() and st["num_skipped"] <= 2
  assert losses[-1] < 0.6 * losses[0], losses
