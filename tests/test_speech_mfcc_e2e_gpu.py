"""The structure of the reference's example_configs/speech2text/lstm_small_1gpu.py at a small width, end to end on
the toy corpus: psf MFCC features (13 coefficients, the config's augmentation block) -> no convolution -> two
unidirectional cudnn_lstm layers -> dense -> CTC, Adam, mixed precision. 13 is not a multiple of 8: the first
recurrent layer zero-pads its input and keeps the logical kernel shape [13 + H, 4H] in checkpoints."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mfcc_ref as mref  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(REPO, "open_seq2seq", "test_utils", "toy_speech_data")
H = 64
KERNEL = "ForwardPass/ds2_encoder/cudnn_lstm/rnn/multi_rnn_cell/cell_0/cudnn_compatible_lstm_cell/kernel"


def _data_layer_params(augment, shuffle):
  p = {"num_audio_features": 13, "input_type": "mfcc", "vocab_file": os.path.join(TOY, "vocab.txt"),
       "dataset_files": [os.path.join(TOY, "toy_data.csv")], "shuffle": shuffle}
  if augment:      # lstm_small_1gpu.py: train_params
    p["augmentation"] = {"time_stretch_ratio": 0.05, "noise_level_min": -90, "noise_level_max": -60}
  return p


def _model(logdir):
  from openseq2seq_amd.data.speech2text.speech2text import Speech2TextDataLayer
  from openseq2seq_amd.decoders.fc_decoders import FullyConnectedCTCDecoder
  from openseq2seq_amd.encoders.ds2_encoder import DeepSpeech2Encoder
  from openseq2seq_amd.losses.ctc_loss import CTCLoss
  from openseq2seq_amd.models.speech2text import Speech2Text
  from openseq2seq_amd.optimizers.lr_policies import exp_decay
  params = dict(
      random_seed=0, use_horovod=False, num_gpus=1, batch_size_per_gpu=4, max_steps=2, logdir=logdir,
      optimizer="Adam", optimizer_params={}, lr_policy=exp_decay,
      lr_policy_params={"learning_rate": 0.001, "begin_decay_at": 0, "decay_steps": 500, "decay_rate": 0.9,
                        "use_staircase_decay": True, "min_lr": 1e-8},
      dtype="mixed", max_grad_norm=0.25, loss_scaling="Backoff",
      encoder=DeepSpeech2Encoder,
      encoder_params={"conv_layers": [], "num_rnn_layers": 2, "rnn_cell_dim": H, "use_cudnn_rnn": True,
                      "rnn_type": "cudnn_lstm", "rnn_unidirectional": True, "row_conv": False, "n_hidden": H,
                      "dropout_keep_prob": 0.5, "activation_fn": "relu", "data_format": "channels_first"},
      decoder=FullyConnectedCTCDecoder, decoder_params={"use_language_model": False},
      loss=CTCLoss, loss_params={},
      data_layer=Speech2TextDataLayer, data_layer_params=_data_layer_params(augment=True, shuffle=True))
  return Speech2Text(params, mode="train").compile()


def test_data_layer_features_match_the_yardstick(monkeypatch):
  """Augmentation off: the batch the data layer feeds is psf.mfcc of the wav files (bf16 output: the bounds of the
  DeepSpeech2 data-layer test in tests/test_psf_spectrogram_gpu.py)."""
  from openseq2seq_amd.data.speech2text.speech2text import Speech2TextDataLayer
  from openseq2seq_amd.data.speech2text.speech_utils import PsfMfccFrontEnd, read_wav
  monkeypatch.chdir(REPO)               # the toy csv names its wav files relative to the repository root
  dl = Speech2TextDataLayer(dict(_data_layer_params(augment=False, shuffle=False), mode="eval", batch_size=4),
                            None, 1, 0)
  batch = next(iter(dl.iterate_batches(torch.device("cuda:0"))))
  feats, frames = batch["source_tensors"]
  torch.cuda.synchronize()
  assert isinstance(dl._front, PsfMfccFrontEnd)
  assert feats.dtype == torch.bfloat16 and feats.shape[0] == 4 and feats.shape[2] == 13 and feats.shape[1] % 8 == 0
  assert "source_lengths_host" not in batch
  for b in range(4):
    sr, sig = read_wav(dl._files[b][0])
    want, _ = mref.psf_mfcc(sig, sr, 13, pad_to=8)
    assert int(frames[b]) == want.shape[0]
    np.testing.assert_allclose(feats[b, :want.shape[0]].float().cpu().numpy(), want, atol=2e-2, rtol=8e-3)
    assert not feats[b, want.shape[0]:].float().any()


def test_two_train_steps_and_the_logical_checkpoint_shape(tmp_path, monkeypatch):
  from openseq2seq_amd.parts.tape import Tape
  from openseq2seq_amd.utils import checkpoint
  monkeypatch.chdir(REPO)
  model = _model(str(tmp_path / "log"))
  wx = model.store.params[[p.name for p in model.store.params].index("ForwardPass/ds2_encoder/cudnn_lstm/layer_0/fw/wx_0")]
  assert wx.shape == (1, 4 * H, 16) and wx.logical_in == 13
  batches = model.get_data_layer().iterate_batches(model._device, seed=0)
  before = model.store.master.clone()
  for _ in range(2):
    batch = next(batches)
    assert batch["source_tensors"][0].shape[2] == 13
    loss = model.train_step(batch)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and float(loss.cpu()[0]) > 0
  assert model.train_op.read_state()["num_skipped"] == 0
  assert torch.isfinite(model.store.master).all() and not torch.equal(before, model.store.master)
  # every gradient of one more forward / backward pass (no update) is finite, and some of every variable's are set
  model.store.zero_grads()
  tape = Tape()
  loss = model._forward_backward(next(batches), tape)
  tape.backward()
  torch.cuda.synchronize()
  assert torch.isfinite(loss).all()
  for p in model.store.params:
    assert torch.isfinite(p.grad).all(), p.name
    assert p.grad.abs().max() > 0, p.name
  assert not wx.master[:, :, 13:].any() and not wx.grad[:, :, 13:].any()       # the padding columns stay zero
  assert wx.master[:, :, :13].abs().max() > 0
  # checkpoint: the first layer's kernel under its logical shape, and back
  prefix = checkpoint.save(model, str(tmp_path / "ckpt"))
  data = checkpoint.open_checkpoint(prefix)
  assert tuple(np.asarray(data[KERNEL]).shape) == (13 + H, 4 * H)
  assert tuple(np.asarray(data[checkpoint.MASTER_PREFIX + KERNEL]).shape) == (13 + H, 4 * H)
  assert tuple(np.asarray(data[KERNEL.replace("cell_0", "cell_1")]).shape) == (H + H, 4 * H)
  other = _model(str(tmp_path / "log2"))
  other.store.master.mul_(0.5)                                                 # (same seed: make the two differ)
  other.store.master[wx.offset:wx.offset + wx.numel].fill_(1.0)               # ... the padding columns too
  assert checkpoint.load(other, prefix) == []
  torch.cuda.synchronize()
  checked = 0
  for p, q in zip(model.store.params, other.store.params):
    assert p.name == q.name
    if p.name.endswith(("/wx_0", "/wh")):       # (a checkpoint holds b_W + b_R: the biases come back as halves)
      assert torch.equal(p.master, q.master), p.name
      checked += 1
  assert checked == 4 and not other.store.params[wx.index].master[:, :, 13:].any()
